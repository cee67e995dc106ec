// slm_attn_fp8_hip.cpp -- see slm_attn_fp8_hip.h.  Pure host code: tensors are unpacked and handed to the C ABI on
// torch's current HIP stream.
#include "slm_attn_fp8_hip.h"

#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/hip/HIPGraphsC10Utils.h>

#include <algorithm>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "slm_hip.h"

namespace {

int t_code(const torch::Tensor& t) {
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16 || t.scalar_type() == torch::kHalf,
              "slm: only fp16 / bf16 activations are supported, got ", t.scalar_type());
  return t.scalar_type() == torch::kBFloat16 ? SLM_BF16 : SLM_F16;
}

void* stream_of(const torch::Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

void ok(int rc, const char* what) {
  TORCH_CHECK(rc == SLM_OK, what, " failed: ", slm_status_string(rc), " (", rc, ")",
              rc == SLM_ERR_LAUNCH ? slm_last_hip_error() : "");
}

void check_cache(const torch::Tensor& c, const char* what) {
  TORCH_CHECK(c.dim() == 3 && c.element_size() == 1 && c.stride(-1) == 1, what,
              ": [n_slots, n_kv_heads, head_dim] of e4m3 codes (one byte per element)");
}

const float* scale_ptr(const torch::Tensor& s, int64_t n_kv_heads, const char* what) {
  TORCH_CHECK(s.scalar_type() == torch::kFloat32 && s.is_contiguous() && s.numel() == n_kv_heads && s.is_cuda(), what,
              ": contiguous fp32 [n_kv_heads] on the device");
  return s.const_data_ptr<float>();
}

// one growable split-KV scratch per device: a buffer that a kernel ever saw is never released (a captured graph keeps
// its address), growth at least doubles and is refused during capture
std::mutex g_mu;
std::unordered_map<int, torch::Tensor> g_ws;
std::vector<torch::Tensor> g_retired;

torch::Tensor scratch(const torch::Tensor& like, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto& ws = g_ws[like.device().index()];
  if (!ws.defined() || static_cast<size_t>(ws.nbytes()) < bytes) {
    TORCH_CHECK(c10::hip::currentStreamCaptureStatusMayInitCtx() == c10::hip::CaptureStatus::None,
                "slm: the fp8 attention workspace must exist before graph capture (need ", bytes, " bytes)");
    size_t size = std::max<size_t>(bytes, 1 << 20);
    if (ws.defined()) {
      size = std::max<size_t>(size, 2 * static_cast<size_t>(ws.nbytes()));
      g_retired.push_back(ws);
    }
    ws = torch::empty({static_cast<int64_t>(size)}, torch::dtype(torch::kUInt8).device(like.device()));
  }
  return ws;
}

}  // namespace

namespace slm {

void set_kv_cache_fp8(const torch::Tensor& slot_ids, const torch::Tensor& keys, const torch::Tensor& values,
                      torch::Tensor& key_cache, torch::Tensor& value_cache, const torch::Tensor& k_scale,
                      const torch::Tensor& v_scale) {
  TORCH_CHECK(keys.dim() == 3 && keys.sizes() == values.sizes() && keys.scalar_type() == values.scalar_type());
  TORCH_CHECK(keys.stride(-1) == 1 && keys.stride(-2) == keys.size(-1));
  TORCH_CHECK(values.stride(-1) == 1 && values.stride(-2) == values.size(-1));
  check_cache(key_cache, "key_cache");
  check_cache(value_cache, "value_cache");
  TORCH_CHECK(key_cache.is_contiguous() && value_cache.is_contiguous() && key_cache.size(1) == keys.size(1) &&
              key_cache.size(2) == keys.size(2) && value_cache.sizes() == key_cache.sizes());
  TORCH_CHECK(slot_ids.scalar_type() == torch::kInt32 && slot_ids.is_contiguous() && slot_ids.numel() == keys.size(0));
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(keys.device());
  ok(slm_kv_fp8_append(slot_ids.const_data_ptr<int32_t>(), keys.const_data_ptr(), values.const_data_ptr(),
                       keys.stride(0), values.stride(0), scale_ptr(k_scale, keys.size(1), "k_scale"),
                       scale_ptr(v_scale, keys.size(1), "v_scale"), key_cache.mutable_data_ptr(),
                       value_cache.mutable_data_ptr(), keys.size(0), static_cast<int32_t>(keys.size(1)),
                       static_cast<int32_t>(keys.size(2)), t_code(keys), stream_of(keys)),
     "slm_kv_fp8_append");
}

void paged_kv_fp8_attention(torch::Tensor& out, const torch::Tensor& query, const torch::Tensor& key_cache,
                            const torch::Tensor& value_cache, const torch::Tensor& q_cu_lens,
                            const torch::Tensor& kv_cu_lens, const torch::Tensor& block_table,
                            const torch::Tensor& block_cu_lens, const std::optional<torch::Tensor>& alibi_slopes,
                            int block_size, int max_q_len, int max_kv_len, float sm_scale,
                            const torch::Tensor& k_scale, const torch::Tensor& v_scale, float logits_soft_cap,
                            int sliding_window, int num_splits) {
  TORCH_CHECK(query.dim() == 3 && out.dim() == 3 && out.scalar_type() == query.scalar_type() &&
              query.stride(-1) == 1 && out.stride(-1) == 1);
  check_cache(key_cache, "key_cache");
  check_cache(value_cache, "value_cache");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(query.device());
  slm_attn_fp8_args a{};
  a.out = out.mutable_data_ptr();
  a.query = query.const_data_ptr();
  a.key_cache = key_cache.const_data_ptr();
  a.value_cache = value_cache.const_data_ptr();
  a.o_stride[0] = out.stride(0); a.o_stride[1] = out.stride(1);
  a.q_stride[0] = query.stride(0); a.q_stride[1] = query.stride(1);
  a.k_stride[0] = key_cache.stride(0); a.k_stride[1] = key_cache.stride(1);
  a.v_stride[0] = value_cache.stride(0); a.v_stride[1] = value_cache.stride(1);
  a.q_cu_lens = q_cu_lens.const_data_ptr<int32_t>();
  a.kv_cu_lens = kv_cu_lens.const_data_ptr<int32_t>();
  a.block_table = block_table.const_data_ptr<int32_t>();
  a.block_cu_lens = block_cu_lens.const_data_ptr<int32_t>();
  // (the library refuses alibi for this kernel: SLM_ERR_UNSUPPORTED)
  a.alibi_slopes = alibi_slopes.has_value() ? alibi_slopes.value().const_data_ptr<float>() : nullptr;
  a.dtype = t_code(query);
  a.batch_size = static_cast<int32_t>(q_cu_lens.size(0) - 1);
  a.n_tokens = static_cast<int32_t>(query.size(0));
  a.n_heads = static_cast<int32_t>(query.size(1));
  a.n_kv_heads = static_cast<int32_t>(key_cache.size(1));
  a.head_dim = static_cast<int32_t>(query.size(2));
  a.block_size = block_size;
  a.max_q_len = max_q_len;
  a.max_kv_len = max_kv_len;
  a.sm_scale = sm_scale;
  a.logits_soft_cap = logits_soft_cap;
  a.sliding_window = sliding_window;
  a.num_splits = num_splits;
  a.k_scale = scale_ptr(k_scale, a.n_kv_heads, "k_scale");
  a.v_scale = scale_ptr(v_scale, a.n_kv_heads, "v_scale");
  slm_attn_fp8_plan_info info;
  ok(slm_paged_kv_fp8_attention_plan(&a, &info), "slm_paged_kv_fp8_attention_plan");
  if (a.n_tokens == 0 || a.batch_size == 0) return;
  torch::Tensor ws;
  if (info.workspace_bytes > 0) {
    ws = scratch(query, info.workspace_bytes);
    a.workspace = ws.mutable_data_ptr();
    a.workspace_bytes = ws.nbytes();
  }
  ok(slm_paged_kv_fp8_attention(&a, stream_of(query)), "slm_paged_kv_fp8_attention");
}

}  // namespace slm
