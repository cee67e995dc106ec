// slm_attn_fp8_hip.h -- the fp8 (e4m3) paged KV cache on the HIP kernels (include/slm_hip.h section 27): two thin free
// functions over slm_kv_fp8_append and slm_paged_kv_fp8_attention, with the argument order of llm::kernel::set_kv_cache
// and llm::paged_kv_varlen_mha plus the scales.  Caches are [n_slots, n_kv_heads, head_dim] of e4m3 codes
// (torch::kFloat8_e4m3fn or torch::kUInt8), k_scale / v_scale fp32 [n_kv_heads] on the device.
#pragma once
#include <optional>

#include <torch/torch.h>

namespace slm {

void set_kv_cache_fp8(const torch::Tensor& slot_ids, const torch::Tensor& keys, const torch::Tensor& values,
                      torch::Tensor& key_cache, torch::Tensor& value_cache, const torch::Tensor& k_scale,
                      const torch::Tensor& v_scale);

// writes `out`; the split-KV workspace is one growable buffer per device, never released and never grown during
// stream capture (warm the call up first)
void paged_kv_fp8_attention(torch::Tensor& out, const torch::Tensor& query, const torch::Tensor& key_cache,
                            const torch::Tensor& value_cache, const torch::Tensor& q_cu_lens,
                            const torch::Tensor& kv_cu_lens, const torch::Tensor& block_table,
                            const torch::Tensor& block_cu_lens, const std::optional<torch::Tensor>& alibi_slopes,
                            int block_size, int max_q_len, int max_kv_len, float sm_scale,
                            const torch::Tensor& k_scale, const torch::Tensor& v_scale, float logits_soft_cap = 0.f,
                            int sliding_window = -1, int num_splits = 0);

}  // namespace slm
