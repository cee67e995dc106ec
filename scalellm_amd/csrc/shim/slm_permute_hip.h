// slm_permute_hip.h -- the MoE token permutation at the libtorch boundary, on top of the C ABI's section 14
// (include/slm_hip.h; csrc/permute.hip):
//   llm::kernel::moe::permute_with_index_map, unpermute_with_index_map   src/kernels/moe/permutation_index_kernel.cu
//   llm::kernel::moe::permute_with_mask_map, unpermute_with_mask_map     src/kernels/moe/permutation_mask_kernel.cu
// with exactly the reference's signatures, so its callers (src/layers/moe/) compile unchanged.  Everything runs on
// torch's current HIP stream and nothing synchronises with the host.  Differences in the values: ids outside the
// kernels' expert range take no row (the reference sorts whatever it is given), and the un-permute sums in fp32
// with one rounding where the reference accumulates in T.
// Python mirror: scalellm_amd/kernels.py (same kernels, same arguments: bit-identical results).
#pragma once
#include <torch/torch.h>

#include <tuple>

namespace llm::kernel::moe {

// -> (permuted_tokens [n_tokens * topk, dim] sorted by (expert, flat index), row_id_map [topk * n_tokens] int32)
std::tuple<torch::Tensor, torch::Tensor> permute_with_index_map(torch::Tensor tokens,   // [n_tokens, dim]
                                                                torch::Tensor indices   // [n_tokens, topk] int32
);

torch::Tensor unpermute_with_index_map(torch::Tensor permuted_tokens,  // [n_permuted_tokens, dim]
                                       torch::Tensor row_id_map,       // [topk, n_tokens]
                                       torch::Tensor probs             // [n_tokens, topk]
);

// -> (permuted_tokens [n_tokens * topk, dim] sorted by (expert, token), row_id_map [n_experts, n_tokens] int32)
std::tuple<torch::Tensor, torch::Tensor> permute_with_mask_map(torch::Tensor tokens,       // [n_tokens, dim]
                                                               torch::Tensor routing_map,  // [n_tokens, n_experts] bool
                                                               int64_t topk);

torch::Tensor unpermute_with_mask_map(torch::Tensor permuted_tokens,  // [n_permuted_tokens, dim]
                                      torch::Tensor row_id_map,       // [n_experts, n_tokens]
                                      torch::Tensor probs             // [n_tokens, n_experts]
);

}  // namespace llm::kernel::moe
