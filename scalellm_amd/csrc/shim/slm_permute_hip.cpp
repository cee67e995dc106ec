// slm_permute_hip.cpp -- see slm_permute_hip.h.  Host code only: tensors are unpacked into the C ABI's arguments
// and handed to the slm_permute_* / slm_unpermute_rows entry points on torch's current HIP stream.
#include "slm_permute_hip.h"

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include "slm_hip.h"

namespace {

constexpr int32_t kMaxExperts = 1024;  // the ABI's upper bound: the reference's index form is not told n_experts

void check(int rc, const char* what) {
  TORCH_CHECK(rc == SLM_OK, what, " failed: ", slm_status_string(rc), " (", rc, ")",
              rc == SLM_ERR_LAUNCH ? slm_last_hip_error() : "");
}

void* stream_of(const torch::Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

int dtype_code(const torch::Tensor& t) {
  if (t.scalar_type() == torch::kBFloat16) return SLM_BF16;
  if (t.scalar_type() == torch::kHalf) return SLM_F16;
  if (t.scalar_type() == torch::kFloat) return SLM_F32;
  TORCH_CHECK(false, "slm permute: fp16 / bf16 / fp32 rows only, got ", t.scalar_type());
  return -1;
}

void check_rows(const torch::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 2 && t.is_contiguous(), "slm permute: ", what,
              " must be a contiguous GPU [rows, dim] tensor");
}

torch::Tensor permute_rows(const torch::Tensor& tokens, const torch::Tensor& row_id_map, int64_t n_maps,
                           int64_t rows) {
  auto permuted = torch::empty({rows, tokens.size(1)}, tokens.options());
  check(slm_permute_rows(permuted.data_ptr(), tokens.data_ptr(), row_id_map.const_data_ptr<int32_t>(), tokens.size(0),
                         static_cast<int32_t>(n_maps), tokens.size(1), rows, dtype_code(tokens), stream_of(tokens)),
        "slm_permute_rows");
  return permuted;
}

torch::Tensor unpermute_rows(const torch::Tensor& permuted, const torch::Tensor& row_id_map,
                             const torch::Tensor& probs, int64_t n_tokens, int64_t n_maps) {
  check_rows(permuted, "permuted_tokens");
  TORCH_CHECK(row_id_map.is_cuda() && row_id_map.scalar_type() == torch::kInt && row_id_map.is_contiguous() &&
                  row_id_map.numel() == n_tokens * n_maps,
              "slm permute: row_id_map must be a contiguous int32 GPU tensor of n_maps * n_tokens entries");
  TORCH_CHECK(probs.is_cuda() && probs.is_contiguous() && probs.numel() == n_tokens * n_maps &&
                  (probs.scalar_type() == torch::kFloat || probs.scalar_type() == permuted.scalar_type()),
              "slm permute: probs must be contiguous [n_tokens, n_maps], fp32 or of the tokens' dtype");
  auto out = torch::empty({n_tokens, permuted.size(1)}, permuted.options());
  check(slm_unpermute_rows(out.data_ptr(), permuted.data_ptr(), row_id_map.const_data_ptr<int32_t>(),
                           probs.data_ptr(), dtype_code(probs), n_tokens, static_cast<int32_t>(n_maps),
                           permuted.size(1), permuted.size(0), dtype_code(permuted), stream_of(permuted)),
        "slm_unpermute_rows");
  return out;
}

}  // namespace

namespace llm::kernel::moe {

std::tuple<torch::Tensor, torch::Tensor> permute_with_index_map(torch::Tensor tokens, torch::Tensor indices) {
  check_rows(tokens, "tokens");
  TORCH_CHECK(indices.is_cuda() && indices.dim() == 2 && indices.scalar_type() == torch::kInt &&
                  indices.is_contiguous() && indices.size(0) == tokens.size(0),
              "slm permute: indices must be a contiguous int32 GPU [n_tokens, topk] tensor");
  const int64_t n_tokens = indices.size(0), topk = indices.size(1);
  auto row_id_map = torch::empty({topk * n_tokens}, indices.options());
  check(slm_permute_index_map(indices.const_data_ptr<int32_t>(), n_tokens, static_cast<int32_t>(topk), kMaxExperts,
                              row_id_map.data_ptr<int32_t>(), nullptr, stream_of(tokens)),
        "slm_permute_index_map");
  return {permute_rows(tokens, row_id_map, topk, n_tokens * topk), row_id_map};
}

torch::Tensor unpermute_with_index_map(torch::Tensor permuted_tokens, torch::Tensor row_id_map, torch::Tensor probs) {
  TORCH_CHECK(probs.dim() == 2, "slm permute: probs must be [n_tokens, topk]");
  return unpermute_rows(permuted_tokens, row_id_map, probs, probs.size(0), probs.size(1));
}

std::tuple<torch::Tensor, torch::Tensor> permute_with_mask_map(torch::Tensor tokens, torch::Tensor routing_map,
                                                               int64_t topk) {
  check_rows(tokens, "tokens");
  TORCH_CHECK(routing_map.is_cuda() && routing_map.dim() == 2 && routing_map.scalar_type() == torch::kBool &&
                  routing_map.is_contiguous() && routing_map.size(0) == tokens.size(0) && topk >= 0,
              "slm permute: routing_map must be a contiguous bool GPU [n_tokens, n_experts] tensor");
  const int64_t n_tokens = routing_map.size(0), n_experts = routing_map.size(1);
  auto row_id_map = torch::empty({n_experts, n_tokens}, tokens.options().dtype(torch::kInt));
  check(slm_permute_mask_map(reinterpret_cast<const uint8_t*>(routing_map.const_data_ptr<bool>()), n_tokens,
                             static_cast<int32_t>(n_experts), row_id_map.data_ptr<int32_t>(), nullptr, nullptr,
                             stream_of(tokens)),
        "slm_permute_mask_map");
  return {permute_rows(tokens, row_id_map, n_experts, n_tokens * topk), row_id_map};
}

torch::Tensor unpermute_with_mask_map(torch::Tensor permuted_tokens, torch::Tensor row_id_map, torch::Tensor probs) {
  TORCH_CHECK(row_id_map.dim() == 2, "slm permute: row_id_map must be [n_experts, n_tokens]");
  return unpermute_rows(permuted_tokens, row_id_map, probs, row_id_map.size(1), row_id_map.size(0));
}

}  // namespace llm::kernel::moe
