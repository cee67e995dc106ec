// slm_moe_hip.h -- the mixture-of-experts operators at the libtorch boundary, on top of the C ABI's section 10
// (include/slm_hip.h; csrc/moe.hip, csrc/w4_moe.hip, csrc/moe_gemm.hip).
//
//   llm::kernel::topk_softmax, llm::kernel::grouped_topk_sigmoid      src/kernels/moe/topk_softmax_kernel.cu:272,
//                                                                      grouped_topk_sigmoid_kernel.cu:280
//   llm::kernel::moe::permute_align_block, llm::kernel::moe::sum_out  src/kernels/moe/align_block_kernel.cu:192, 242
// with exactly the reference's signatures, so its callers compile unchanged, and
//   slm::moe_w4_grouped_gemm   the grouped int4 GEMM over stacked packed experts (the reference's grouped GEMM,
//                              src/kernels/gemm/, is a dense fp16 / bf16 kernel; int4 experts have no counterpart).
//   slm::moe_grouped_gemm      that dense fp16 / bf16 grouped GEMM over W[e, n, k].
//   slm::moe_fp8_grouped_gemm  the same over fp8 (e4m3) experts with channel scales (section 16, csrc/moe_gemm.hip).
//   slm::moe_mxfp4_grouped_gemm  the same over OCP MXFP4 experts with e8m0 block scales (section 21, csrc/moe_gemm.hip).
//   slm::moe_router            the fused router: gate GEMM + routing in one launch (section 17, csrc/moe_router.hip).
// Everything runs on torch's current HIP stream and nothing synchronises with the host.
// Python mirror: scalellm_amd/kernels.py (same kernels, same arguments: bit-identical results).
#pragma once
#include <torch/torch.h>

namespace llm::kernel {

// the k largest logits per token (ties: the lower expert id), weights = softmax over all experts at those
void topk_softmax(const torch::Tensor& gating_logits,  // [n_tokens, n_experts] fp32
                  torch::Tensor& topk_weights,         // [n_tokens, topk] fp32
                  torch::Tensor& topk_indices          // [n_tokens, topk] int32
);

void grouped_topk_sigmoid(const torch::Tensor& gating_logits,    // [n_tokens, n_experts] fp32
                          const torch::Tensor& correction_bias,  // [n_experts] fp32
                          const int n_expert_groups, const int topk_group, const int topk, float scaling_factor,
                          torch::Tensor& topk_weights,  // [n_tokens, topk]
                          torch::Tensor& topk_indices   // [n_tokens, topk]
);

namespace moe {

// sorted_token_idxes / experts_ids must hold at least slm_moe_align_capacity(n_flat, n_experts, block_size) entries;
// the kernel writes the padding entries of [0, n_padded) itself, an expert's indices in ascending order
void permute_align_block(torch::Tensor topk_ids,  // [n_tokens, topk] int32
                         int64_t n_experts, int64_t block_size,
                         torch::Tensor sorted_token_idxes,  // [n_padded_permuted_tokens+]
                         torch::Tensor experts_ids,         // [n_blocks+]
                         torch::Tensor n_padded_tokens,     // [1]
                         torch::Tensor cu_sum               // [n_experts+1]
);

void sum_out(const torch::Tensor& input,  // [n_tokens, topk, dim]
             torch::Tensor& output);      // [n_tokens, dim]

}  // namespace moe
}  // namespace llm::kernel

namespace slm {

// sum_out with one more row per token, the shared experts' output, added last in the same fp32 accumulation
// (slm_moe_sum_add): bit-identical to sum_out over [n_tokens, topk + 1, dim].  output may be addend.
void moe_sum_add(const torch::Tensor& input,   // [n_tokens, topk, dim]
                 const torch::Tensor& addend,  // [n_tokens, dim]
                 torch::Tensor& output);       // [n_tokens, dim]

// topk_softmax with the k weights divided by their sum (Mixtral's rule)
void moe_topk_softmax(const torch::Tensor& gating_logits, torch::Tensor& topk_weights, torch::Tensor& topk_indices,
                      bool renormalize);

// C[idx] = epilogue(A[idx / a_div] . dequant(W_e)) over the 32-row blocks of permute_align_block(block_size = 32).
// wq [E, K * N / 8], sz [E, (K / group_size) * N] int32: slm_w4_prepack images stacked per expert; format: the
// slm_w4_format they were packed from (| SLM_W4_PAIRED).  row_scale: fp32 [n_flat] or undefined; silu_mul: paired
// experts, c is [n_flat, N / 2].
void moe_w4_grouped_gemm(const torch::Tensor& a, const torch::Tensor& wq, const torch::Tensor& sz, torch::Tensor& c,
                         const torch::Tensor& sorted_token_idxes, const torch::Tensor& expert_ids,
                         const torch::Tensor& n_padded_tokens, int64_t K, int64_t N, int64_t group_size,
                         int64_t a_div, int64_t format, const torch::Tensor& row_scale, bool silu_mul);

// C[idx] = epilogue(A[idx / a_div] . W[e]^T) over unquantised experts w [E, N, K] (the checkpoint layout, k contiguous;
// expert and row strides may exceed the dense ones) -- the reference's grouped GEMM itself.  row_scale: fp32 [n_flat]
// or undefined; silu_mul: rows [0, N/2) of an expert are the gate, [N/2, N) the up projection, c is [n_flat, N / 2].
void moe_grouped_gemm(const torch::Tensor& a, const torch::Tensor& w, torch::Tensor& c,
                      const torch::Tensor& sorted_token_idxes, const torch::Tensor& expert_ids,
                      const torch::Tensor& n_padded_tokens, int64_t a_div, const torch::Tensor& row_scale,
                      bool silu_mul);

// moe_grouped_gemm over fp8 experts (include/slm_hip.h section 16): w8 [E, N, K] float8_e4m3fn (or its bytes as
// uint8), the checkpoint layout; w_scale fp32 [E, N] (one scale per expert and output channel) or undefined (1.0),
// applied to the fp32 accumulator before row_scale and the one rounding.  The rest as moe_grouped_gemm.
void moe_fp8_grouped_gemm(const torch::Tensor& a, const torch::Tensor& w8, const torch::Tensor& w_scale,
                          torch::Tensor& c, const torch::Tensor& sorted_token_idxes, const torch::Tensor& expert_ids,
                          const torch::Tensor& n_padded_tokens, int64_t a_div, const torch::Tensor& row_scale,
                          bool silu_mul);

// moe_grouped_gemm over OCP MXFP4 experts (include/slm_hip.h section 21): w uint8 [E, N, K/2] (two e2m1 codes a byte,
// the low nibble the lower k; expert and row strides multiples of 16), w_scale uint8 [E, N, K/32] e8m0 bytes (any
// stride, any alignment), both required and read as the checkpoint stores them.  The rest as moe_grouped_gemm.
void moe_mxfp4_grouped_gemm(const torch::Tensor& a, const torch::Tensor& w, const torch::Tensor& w_scale,
                            torch::Tensor& c, const torch::Tensor& sorted_token_idxes,
                            const torch::Tensor& expert_ids, const torch::Tensor& n_padded_tokens, int64_t a_div,
                            const torch::Tensor& row_scale, bool silu_mul);

// logits = x [T, hidden] . gate_weight [E, hidden]^T in fp32 and their routing, in one launch: scoring "softmax"
// (renormalize) or "grouped_sigmoid" (correction_bias, n_expert_groups, topk_group, scaling_factor); topk is
// topk_weights.size(1).  correction_bias / logits_out (fp32 [T, E]) may be undefined tensors.
void moe_router(const torch::Tensor& x, const torch::Tensor& gate_weight, torch::Tensor& topk_weights,
                torch::Tensor& topk_indices, const std::string& scoring, bool renormalize,
                const torch::Tensor& correction_bias, int64_t n_expert_groups, int64_t topk_group,
                double scaling_factor, const torch::Tensor& logits_out);

}  // namespace slm
