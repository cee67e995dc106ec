// slm_mla_hip.cpp -- see slm_mla_hip.h.  Host code only: tensors are unpacked into slm_mla_args and handed to the
// slm_mla_* entry points on torch's current HIP stream.
#include "slm_mla_hip.h"

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/hip/HIPGraphsC10Utils.h>

#include <map>
#include <mutex>
#include <vector>

#include "slm_hip.h"

namespace {

void check(int rc, const char* what) {
  TORCH_CHECK(rc == SLM_OK, what, " failed: ", slm_status_string(rc), " (", rc, ")",
              rc == SLM_ERR_LAUNCH ? slm_last_hip_error() : "");
}

void* stream_of(const torch::Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

void check_i32(const torch::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt && t.is_contiguous(), "slm mla: ", what,
              " must be a contiguous int32 GPU tensor");
}

int dtype_code(const torch::Tensor& t) {
  if (t.scalar_type() == torch::kBFloat16) return SLM_BF16;
  if (t.scalar_type() == torch::kHalf) return SLM_F16;
  TORCH_CHECK(false, "slm mla: fp16 / bf16 only, got ", t.scalar_type());
  return -1;
}

// split-KV scratch per device.  A buffer that was handed to a kernel is never released (graphs captured earlier
// replay against its address); growth happens outside capture only.
std::mutex g_ws_mu;
std::map<int, torch::Tensor> g_ws;
std::vector<torch::Tensor> g_ws_retired;

torch::Tensor workspace(size_t need, const torch::Tensor& like) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  const int dev = like.device().index();
  auto it = g_ws.find(dev);
  if (it != g_ws.end() && static_cast<size_t>(it->second.numel()) >= need) return it->second;
  TORCH_CHECK(c10::hip::currentStreamCaptureStatusMayInitCtx() == c10::hip::CaptureStatus::None,
              "slm mla: the split-KV workspace (", need, " bytes) must exist before graph capture: run the call once first");
  size_t size = need > (size_t{1} << 20) ? need : (size_t{1} << 20);
  if (it != g_ws.end()) {
    g_ws_retired.push_back(it->second);
    if (size < 2 * static_cast<size_t>(it->second.numel())) size = 2 * static_cast<size_t>(it->second.numel());
  }
  torch::Tensor ws = torch::empty({static_cast<int64_t>(size)}, torch::dtype(torch::kUInt8).device(like.device()));
  g_ws[dev] = ws;
  return ws;
}

}  // namespace

namespace slm {

void mla_paged_kv(torch::Tensor& out, const torch::Tensor& q, const torch::Tensor& kv_cache, const torch::Tensor& q_rope,
                  const torch::Tensor& k_rope_cache, const torch::Tensor& q_cu_lens, const torch::Tensor& kv_cu_lens,
                  const torch::Tensor& block_table, const torch::Tensor& block_cu_lens, int block_size, int max_q_len,
                  int max_kv_len, float sm_scale) {
  TORCH_CHECK(out.is_cuda() && q.is_cuda() && q_rope.is_cuda() && kv_cache.is_cuda() && k_rope_cache.is_cuda(),
              "slm mla: GPU tensors only");
  TORCH_CHECK(out.dim() == 3 && q.dim() == 3 && q_rope.dim() == 3 && kv_cache.dim() == 2 && k_rope_cache.dim() == 2,
              "slm mla: out / q / q_rope are [n_tokens, n_heads, dim], the caches [n_slots, dim]");
  TORCH_CHECK(out.stride(-1) == 1 && q.stride(-1) == 1 && q_rope.stride(-1) == 1 && kv_cache.stride(-1) == 1 &&
                  k_rope_cache.stride(-1) == 1,
              "slm mla: last dimension must be contiguous");
  TORCH_CHECK(out.scalar_type() == q.scalar_type() && q_rope.scalar_type() == q.scalar_type() &&
                  kv_cache.scalar_type() == q.scalar_type() && k_rope_cache.scalar_type() == q.scalar_type(),
              "slm mla: dtypes must match");
  TORCH_CHECK(out.sizes() == q.sizes() && q_rope.size(0) == q.size(0) && q_rope.size(1) == q.size(1) &&
                  kv_cache.size(1) == q.size(2) && k_rope_cache.size(1) == q_rope.size(2) &&
                  kv_cache.size(0) == k_rope_cache.size(0),
              "slm mla: shape mismatch between out / q / q_rope / caches");
  check_i32(q_cu_lens, "q_cu_lens");
  check_i32(kv_cu_lens, "kv_cu_lens");
  check_i32(block_table, "block_table");
  check_i32(block_cu_lens, "block_cu_lens");
  slm_mla_args a{};
  a.out = out.data_ptr();
  a.q = q.data_ptr();
  a.q_rope = q_rope.data_ptr();
  a.kv_cache = kv_cache.data_ptr();
  a.k_rope_cache = k_rope_cache.data_ptr();
  a.o_stride[0] = out.stride(0);
  a.o_stride[1] = out.stride(1);
  a.q_stride[0] = q.stride(0);
  a.q_stride[1] = q.stride(1);
  a.q_rope_stride[0] = q_rope.stride(0);
  a.q_rope_stride[1] = q_rope.stride(1);
  a.kv_stride = kv_cache.stride(0);
  a.k_rope_stride = k_rope_cache.stride(0);
  a.q_cu_lens = q_cu_lens.const_data_ptr<int32_t>();
  a.kv_cu_lens = kv_cu_lens.const_data_ptr<int32_t>();
  a.block_table = block_table.const_data_ptr<int32_t>();
  a.block_cu_lens = block_cu_lens.const_data_ptr<int32_t>();
  a.dtype = dtype_code(q);
  a.batch_size = static_cast<int32_t>(q_cu_lens.numel() - 1);
  a.n_tokens = static_cast<int32_t>(q.size(0));
  a.n_heads = static_cast<int32_t>(q.size(1));
  a.head_dim = static_cast<int32_t>(q.size(2));
  a.rope_head_dim = static_cast<int32_t>(q_rope.size(2));
  a.block_size = block_size;
  a.max_q_len = max_q_len;
  a.max_kv_len = max_kv_len;
  a.sm_scale = sm_scale;
  if (a.n_tokens == 0 || a.batch_size == 0) return;
  torch::Tensor ws;
  const size_t need = slm_mla_paged_kv_workspace_bytes(&a);
  if (need > 0) {
    ws = workspace(need, q);
    a.workspace = ws.data_ptr();
    a.workspace_bytes = static_cast<size_t>(ws.numel());
  }
  check(slm_mla_paged_kv(&a, stream_of(q)), "slm_mla_paged_kv");
}

void mla_set_kv_cache(const torch::Tensor& slot_ids, const torch::Tensor& kv, const torch::Tensor& k_rope,
                      torch::Tensor& kv_cache, torch::Tensor& k_rope_cache) {
  check_i32(slot_ids, "slot_ids");
  TORCH_CHECK(kv.is_cuda() && k_rope.is_cuda() && kv_cache.is_cuda() && k_rope_cache.is_cuda() && kv.dim() == 2 &&
                  k_rope.dim() == 2 && kv_cache.dim() == 2 && k_rope_cache.dim() == 2 && kv.stride(1) == 1 &&
                  k_rope.stride(1) == 1 && kv_cache.stride(1) == 1 && k_rope_cache.stride(1) == 1,
              "slm mla: set_kv_cache takes 2-D GPU tensors with contiguous rows");
  TORCH_CHECK(k_rope.scalar_type() == kv.scalar_type() && kv_cache.scalar_type() == kv.scalar_type() &&
                  k_rope_cache.scalar_type() == kv.scalar_type(),
              "slm mla: dtypes must match");
  TORCH_CHECK(kv.size(0) == slot_ids.numel() && k_rope.size(0) == slot_ids.numel() && kv.size(1) == kv_cache.size(1) &&
                  k_rope.size(1) == k_rope_cache.size(1),
              "slm mla: set_kv_cache shape mismatch");
  check(slm_mla_set_kv_cache(slot_ids.const_data_ptr<int32_t>(), kv.data_ptr(), k_rope.data_ptr(), kv.stride(0),
                             k_rope.stride(0), kv_cache.data_ptr(), k_rope_cache.data_ptr(), kv_cache.stride(0),
                             k_rope_cache.stride(0), kv.size(0), static_cast<int32_t>(kv.size(1)),
                             static_cast<int32_t>(k_rope.size(1)), dtype_code(kv), stream_of(kv)),
        "slm_mla_set_kv_cache");
}

void mla_rope_append(torch::Tensor q, const torch::Tensor& kv_a, const torch::Tensor& norm_weight, double eps,
                     const torch::Tensor& positions, const torch::Tensor& cos_sin, bool interleaved,
                     const torch::Tensor& slot_ids, torch::Tensor& kv_cache, torch::Tensor& k_rope_cache,
                     int64_t nope_head_dim, const torch::Tensor& partials) {
  check_i32(positions, "positions");
  check_i32(slot_ids, "slot_ids");
  const int64_t T = positions.numel();
  TORCH_CHECK(slot_ids.numel() == T, "slm mla: positions and slot_ids must have one entry per token");
  TORCH_CHECK(kv_cache.is_cuda() && k_rope_cache.is_cuda() && kv_cache.dim() == 2 && k_rope_cache.dim() == 2 &&
                  kv_cache.stride(1) == 1 && k_rope_cache.stride(1) == 1 && kv_cache.size(0) == k_rope_cache.size(0) &&
                  k_rope_cache.scalar_type() == kv_cache.scalar_type(),
              "slm mla: caches [n_slots, latent] and [n_slots, rope] of one dtype with contiguous rows");
  const int64_t latent = kv_cache.size(1), rope = k_rope_cache.size(1);
  const auto dt = kv_cache.scalar_type();
  TORCH_CHECK(norm_weight.is_cuda() && norm_weight.scalar_type() == dt && norm_weight.is_contiguous() &&
                  norm_weight.numel() == latent,
              "slm mla: norm_weight must be a contiguous [latent] tensor of the cache dtype");
  const bool cs_f32 = cos_sin.scalar_type() == torch::kFloat;
  TORCH_CHECK(cos_sin.is_cuda() && cos_sin.is_contiguous() && (cs_f32 || cos_sin.scalar_type() == dt) &&
                  cos_sin.size(-1) == rope,
              "slm mla: cos_sin must be contiguous [max_pos, rope], fp32 or the activation dtype");
  int32_t n_heads = 0;
  if (q.defined() && q.numel() > 0) {
    TORCH_CHECK(q.is_cuda() && q.dim() == 3 && q.size(0) == T && q.scalar_type() == dt && q.stride(2) == 1 &&
                    q.stride(1) == q.size(2) && q.size(2) == nope_head_dim + rope,
                "slm mla: q must be [n_tokens, n_heads, nope + rope], contiguous in its last two dims");
    n_heads = static_cast<int32_t>(q.size(1));
  }
  void* qp = n_heads ? q.data_ptr() : nullptr;
  const int64_t q_ts = n_heads ? q.stride(0) : 0;
  if (partials.defined()) {
    const int64_t n_cols = n_heads * (nope_head_dim + rope) + latent + rope;
    TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == torch::kFloat && partials.is_contiguous() &&
                    partials.dim() == 3 && partials.size(1) == T && partials.size(2) == n_cols,
                "slm mla: partials must be contiguous fp32 [n_splits, n_tokens, n_heads (nope + rope) + latent + rope]");
    check(slm_mla_rope_append_splitk(partials.const_data_ptr<float>(), static_cast<int32_t>(partials.size(0)), qp, q_ts,
                                     norm_weight.data_ptr(), static_cast<float>(eps),
                                     positions.const_data_ptr<int32_t>(), cos_sin.data_ptr(), cs_f32 ? 1 : 0,
                                     interleaved ? 1 : 0, slot_ids.const_data_ptr<int32_t>(), kv_cache.data_ptr(),
                                     k_rope_cache.data_ptr(), kv_cache.stride(0), k_rope_cache.stride(0), T, n_heads,
                                     static_cast<int32_t>(nope_head_dim), static_cast<int32_t>(latent),
                                     static_cast<int32_t>(rope), dtype_code(kv_cache), stream_of(kv_cache)),
          "slm_mla_rope_append_splitk");
    return;
  }
  TORCH_CHECK(kv_a.defined() && kv_a.is_cuda() && kv_a.dim() == 2 && kv_a.size(0) == T && kv_a.size(1) == latent + rope &&
                  kv_a.scalar_type() == dt && kv_a.stride(1) == 1,
              "slm mla: kv_a must be [n_tokens, latent + rope] of the cache dtype with contiguous rows");
  check(slm_mla_rope_append(qp, q_ts, kv_a.data_ptr(), kv_a.stride(0), norm_weight.data_ptr(), static_cast<float>(eps),
                            positions.const_data_ptr<int32_t>(), cos_sin.data_ptr(), cs_f32 ? 1 : 0,
                            interleaved ? 1 : 0, slot_ids.const_data_ptr<int32_t>(), kv_cache.data_ptr(),
                            k_rope_cache.data_ptr(), kv_cache.stride(0), k_rope_cache.stride(0), T, n_heads,
                            static_cast<int32_t>(nope_head_dim), static_cast<int32_t>(latent),
                            static_cast<int32_t>(rope), dtype_code(kv_cache), stream_of(kv_cache)),
        "slm_mla_rope_append");
}

void qk_norm_rope_kv_append(torch::Tensor q, torch::Tensor k, torch::Tensor v, const torch::Tensor& q_norm_weight,
                            const torch::Tensor& k_norm_weight, double eps, const torch::Tensor& positions,
                            const torch::Tensor& cos_sin, bool interleaved, const torch::Tensor& slot_ids,
                            const torch::Tensor& key_cache, const torch::Tensor& value_cache,
                            const torch::Tensor& partials) {
  check_i32(positions, "positions");
  const int64_t T = positions.numel();
  const auto dt = q.scalar_type();
  for (const torch::Tensor* t : {&q, &k, &v})
    TORCH_CHECK(t->is_cuda() && t->dim() == 3 && t->size(0) == T && t->scalar_type() == dt && t->stride(2) == 1 &&
                    t->stride(1) == t->size(2),
                "slm qk_norm: q / k / v must be [n_tokens, heads, head_dim] of one dtype, contiguous in their last "
                "two dims");
  const int64_t D = q.size(2);
  TORCH_CHECK(k.size(2) == D && v.sizes() == k.sizes(), "slm qk_norm: head_dim of q / k / v must match; v like k");
  for (const torch::Tensor* w : {&q_norm_weight, &k_norm_weight})
    TORCH_CHECK(w->is_cuda() && w->scalar_type() == dt && w->is_contiguous() && w->numel() == D,
                "slm qk_norm: the norm weights must be contiguous [head_dim] tensors of the activation dtype");
  const bool cs_f32 = cos_sin.scalar_type() == torch::kFloat;
  TORCH_CHECK(cos_sin.is_cuda() && cos_sin.is_contiguous() && (cs_f32 || cos_sin.scalar_type() == dt),
              "slm qk_norm: cos_sin must be contiguous, fp32 or the activation dtype");
  const bool append = slot_ids.defined();
  if (append) {
    check_i32(slot_ids, "slot_ids");
    TORCH_CHECK(slot_ids.numel() == T, "slm qk_norm: positions and slot_ids must have one entry per token");
    for (const torch::Tensor* c : {&key_cache, &value_cache})
      TORCH_CHECK(c->defined() && c->is_cuda() && c->is_contiguous() && c->scalar_type() == dt && c->dim() == 3 &&
                      c->size(1) == k.size(1) && c->size(2) == D,
                  "slm qk_norm: caches must be contiguous [n_slots, n_kv_heads, head_dim] of the activation dtype");
  }
  const int32_t* sp = append ? slot_ids.const_data_ptr<int32_t>() : nullptr;
  void* kc = append ? key_cache.data_ptr() : nullptr;
  void* vc = append ? value_cache.data_ptr() : nullptr;
  const int32_t H = static_cast<int32_t>(q.size(1)), KV = static_cast<int32_t>(k.size(1));
  if (partials.defined()) {
    TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == torch::kFloat && partials.is_contiguous() &&
                    partials.dim() == 3 && partials.size(1) == T && partials.size(2) == (H + 2 * KV) * D,
                "slm qk_norm: partials must be contiguous fp32 [n_splits, n_tokens, (n_heads + 2 n_kv_heads) head_dim]");
    check(slm_qk_norm_rope_kv_append_splitk(
              partials.const_data_ptr<float>(), static_cast<int32_t>(partials.size(0)), q.data_ptr(), q.stride(0),
              k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), q_norm_weight.data_ptr(), k_norm_weight.data_ptr(),
              static_cast<float>(eps), positions.const_data_ptr<int32_t>(), cos_sin.data_ptr(), cs_f32 ? 1 : 0,
              static_cast<int32_t>(cos_sin.size(-1)), interleaved ? 1 : 0, sp, kc, vc, T, H, KV,
              static_cast<int32_t>(D), dtype_code(q), stream_of(q)),
          "slm_qk_norm_rope_kv_append_splitk");
    return;
  }
  check(slm_qk_norm_rope_kv_append(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                   q_norm_weight.data_ptr(), k_norm_weight.data_ptr(), static_cast<float>(eps),
                                   positions.const_data_ptr<int32_t>(), cos_sin.data_ptr(), cs_f32 ? 1 : 0,
                                   static_cast<int32_t>(cos_sin.size(-1)), interleaved ? 1 : 0, sp, kc, vc, T, H, KV,
                                   static_cast<int32_t>(D), dtype_code(q), stream_of(q)),
        "slm_qk_norm_rope_kv_append");
}

}  // namespace slm
