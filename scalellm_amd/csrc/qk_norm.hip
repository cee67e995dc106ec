// qk_norm.hip -- the QK-norm attention prologue (include/slm_hip.h section 19): what sits between the qkv projection
// GEMM and paged attention in a Qwen3 / Qwen3-MoE layer, in ONE launch:
//   every q head and every k head  n = RMSNorm(x; w, eps) over the head's D values (w = q_norm / k_norm, [D],
//                                  shared by the heads), then n rotated by cos_sin[positions[t]]   -> q / k in place
//   k and v                                                                                        -> cache[slot]
// The arithmetic is the existing kernels' own, shared through headers: rms_sumsq8 / rms_rstd / rms_apply8 and the
// butterfly of rms_norm_kernel (common.h), rope_unit8 (rope.h), slab_sum8 / splitk_sum4 (common.h) -- so the results
// are bit-identical to slm_rms_norm on [T * heads, D] rows, then slm_rope_kv_append (and to the split-K reduce first).
//
// Why the statistic matches: rms_norm_kernel gives vector i of a row to thread i and adds with group_sum<64>, then
// red[0] + red[1] + red[2] + red[3].  For D <= 512 only lanes 0 .. D / 8 - 1 of wave 0 hold non-zero terms: the
// butterfly stages past D / 8 lanes add exact zeros, as do red[1..3].  So a group of G = D / 8 lanes, lane j owning
// vector j, reduced with group_sum<G> (the same first stages), gives the same bits.
//
// Launch shape (mla_glue.hip's).  The unit of work is a WAVE TASK: 64 / G heads per wave (q heads, then k heads,
// mixed within a wave where they meet), then the v-copy vectors, 64 per task.  No LDS, no barrier.  Tasks are
// numbered token-major, four per 256-thread workgroup, so one token already spreads over independent waves.
// Under the (i, i + D / 2) pairing the rotation partner of lane j's values sits in lane j ^ (G / 2) of the same
// group: it is fetched with a cross-lane move of the normalised (T-rounded) vector, and each lane computes the
// rope_unit8 halves it owns.  Under the interleaved pairing the pairs are inside the lane.
#include "common.h"
#include "rope.h"

namespace slm {
namespace {

constexpr int kQkNormWaves = 4;

struct QkNormParams {
  const float* part;  // slab form: [n_splits, T, N] fp32, else nullptr
  int64_t slab, N;
  uint16_t* q;
  uint16_t* k;
  uint16_t* v;
  const uint16_t* qw;
  const uint16_t* kw;
  const int* positions;
  const void* cos_sin;
  const int* slot_ids;  // or nullptr: no append
  uint16_t* kc;
  uint16_t* vc;
  int64_t q_ts, k_ts, v_ts, T;
  float eps;
  int n_splits, interleaved, n_heads, n_kv_heads, head_tasks, tasks_per_token;
};

template <typename T, typename CS, int D, bool PART>
__global__ void __launch_bounds__(64 * kQkNormWaves) qk_norm_rope_kv_append_kernel(const QkNormParams p) {
  constexpr int G = D / 8;     // lanes per head, one 16-byte vector each
  constexpr int HPW = 64 / G;  // heads per wave
  constexpr int HALF = D / 2;
  const int lane = threadIdx.x & 63;
  const int64_t task = (int64_t)blockIdx.x * kQkNormWaves + (threadIdx.x >> 6);
  const int64_t tok = task / p.tasks_per_token;
  if (tok >= p.T) return;  // wave-uniform; no barrier below
  const int sub = (int)(task - tok * p.tasks_per_token);
  const int64_t slot = p.slot_ids ? (int64_t)p.slot_ids[tok] : -1;
  const int64_t row = (int64_t)p.n_kv_heads * D;  // cache slot stride
  const float* prow = PART ? p.part + tok * p.N : nullptr;

  if (sub < p.head_tasks) {  // ---- HPW heads: RMSNorm, rotation, in place (k also to its slot)
    const int n_rot = p.n_heads + p.n_kv_heads;
    const int hg = sub * HPW + lane / G;
    const int j = lane % G;           // this lane's vector of the head
    const bool valid = hg < n_rot;
    const int h = min(hg, n_rot - 1);  // unconditional loads: head clamped, stores masked
    const bool is_k = h >= p.n_heads;
    const int hh = is_k ? h - p.n_heads : h;
    const u32x4 wv = *reinterpret_cast<const u32x4*>((is_k ? p.kw : p.qw) + j * 8);
    uint16_t* dst = is_k ? p.k + tok * p.k_ts + (int64_t)hh * D : p.q + tok * p.q_ts + (int64_t)hh * D;
    u32x4 a;
    if constexpr (PART) a = slab_sum8<T>(prow + (int64_t)h * D + j * 8, p.slab, p.n_splits);  // k follows q
    else a = *reinterpret_cast<const u32x4*>(dst + j * 8);
    const CS* cs = reinterpret_cast<const CS*>(p.cos_sin) + (int64_t)p.positions[tok] * D;
    float f[8];
    unpack8<T>(a, f);
    const float ss = group_sum<G>(rms_sumsq8(f, 0.f));
    const float rs = rms_rstd(ss, (float)D, p.eps);
    const u32x4 n = rms_apply8<T>(f, rs, wv);  // slm_rms_norm's bits, in T
    float nf[8], o[8];
    unpack8<T>(n, nf);
    if (p.interleaved) {  // unit j: pairs (2i, 2i + 1) of the lane's own 8 values
      const float na[4] = {nf[0], nf[1], nf[2], nf[3]}, nb[4] = {nf[4], nf[5], nf[6], nf[7]};
      float oa[4], ob[4];
      rope_unit8<T>(na, nb, cs, HALF, j, 1, oa, ob);
#pragma unroll
      for (int e = 0; e < 4; ++e) { o[e] = oa[e]; o[4 + e] = ob[e]; }
    } else {  // pairs (i, i + HALF): the partner vector is lane j ^ (G / 2)'s
      u32x4 m;
      m.x = __shfl_xor(n.x, G / 2, 64); m.y = __shfl_xor(n.y, G / 2, 64);
      m.z = __shfl_xor(n.z, G / 2, 64); m.w = __shfl_xor(n.w, G / 2, 64);
      float mf[8];
      unpack8<T>(m, mf);
      const bool lo = j < G / 2;  // this lane holds dims [8j, 8j + 8) below HALF: units 2j, 2j + 1 (a side)
      const int u0 = 2 * (lo ? j : j - G / 2);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        float xa[4], xb[4], oa[4], ob[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          xa[i] = lo ? nf[4 * e + i] : mf[4 * e + i];
          xb[i] = lo ? mf[4 * e + i] : nf[4 * e + i];
        }
        rope_unit8<T>(xa, xb, cs, HALF, u0 + e, 0, oa, ob);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[4 * e + i] = lo ? oa[i] : ob[i];
      }
    }
    u32x4 r;
    r.x = pack2<T>(o[0], o[1]); r.y = pack2<T>(o[2], o[3]);
    r.z = pack2<T>(o[4], o[5]); r.w = pack2<T>(o[6], o[7]);
    if (!valid) return;
    *reinterpret_cast<u32x4*>(dst + j * 8) = r;
    if (is_k && slot >= 0) *reinterpret_cast<u32x4*>(p.kc + slot * row + (int64_t)hh * D + j * 8) = r;
    return;
  }
  // ---- v: 8 columns per lane, to the cache slot (slab form: also to v)
  const int i = (sub - p.head_tasks) * 64 + lane;
  if (i >= (int)(row / 8) || (!PART && slot < 0)) return;
  u32x4 a;
  if constexpr (PART) {
    a = slab_sum8<T>(prow + (int64_t)(p.n_heads + p.n_kv_heads) * D + i * 8, p.slab, p.n_splits);
    *reinterpret_cast<u32x4*>(p.v + tok * p.v_ts + i * 8) = a;
  } else {
    a = *reinterpret_cast<const u32x4*>(p.v + tok * p.v_ts + i * 8);
  }
  if (slot >= 0) *reinterpret_cast<u32x4*>(p.vc + slot * row + i * 8) = a;
}

inline bool stride16(int64_t elems) { return (elems & 7) == 0; }

template <typename TT, typename CS, int D>
void qk_norm_dispatch(const QkNormParams& p, bool slabs, dim3 g, dim3 blk, hipStream_t st) {
  if (slabs) hipLaunchKernelGGL((qk_norm_rope_kv_append_kernel<TT, CS, D, true>), g, blk, 0, st, p);
  else hipLaunchKernelGGL((qk_norm_rope_kv_append_kernel<TT, CS, D, false>), g, blk, 0, st, p);
}

int qk_norm_launch(const float* partials, int32_t n_splits, void* q, int64_t q_ts, void* k, int64_t k_ts, void* v,
                   int64_t v_ts, const void* q_norm_weight, const void* k_norm_weight, float eps,
                   const int32_t* positions, const void* cos_sin, int32_t cos_sin_is_f32, int32_t rot_dim,
                   int32_t interleaved, const int32_t* slot_ids, void* key_cache, void* value_cache,
                   int64_t n_tokens, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, int32_t dtype, bool slabs,
                   void* stream) {
  if (n_tokens < 0 || n_tokens > 0x7fffffffLL || n_heads < 1 || n_kv_heads < 1 || head_dim < 0 || rot_dim < 0)
    return SLM_ERR_INVALID_ARG;
  if (n_tokens == 0) return SLM_OK;
  if ((slabs && (!partials || n_splits < 1)) || !q || !k || !v || !q_norm_weight || !k_norm_weight || !positions ||
      !cos_sin || (slot_ids && (!key_cache || !value_cache)))
    return SLM_ERR_INVALID_ARG;
  if (dtype != SLM_F16 && dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if ((head_dim != 64 && head_dim != 128 && head_dim != 256) || rot_dim != head_dim) return SLM_ERR_UNSUPPORTED;
  if (!aligned16(partials) || !aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(q_norm_weight) ||
      !aligned16(k_norm_weight) || !aligned16(cos_sin) || !aligned16(key_cache) || !aligned16(value_cache) ||
      !stride16(q_ts) || !stride16(k_ts) || !stride16(v_ts))
    return SLM_ERR_ALIGNMENT;
  const int64_t hpw = 512 / head_dim;
  const int64_t head_tasks = ((int64_t)n_heads + n_kv_heads + hpw - 1) / hpw;
  const int64_t v_tasks = (slabs || slot_ids) ? ((int64_t)n_kv_heads * head_dim / 8 + 63) / 64 : 0;
  const int64_t tasks_per_token = head_tasks + v_tasks;
  const int64_t grid = (n_tokens * tasks_per_token + kQkNormWaves - 1) / kQkNormWaves;
  if (tasks_per_token > 0x7fffffffLL || grid > 0x7fffffffLL) return SLM_ERR_UNSUPPORTED;
  QkNormParams p;
  p.part = slabs ? partials : nullptr;
  p.N = ((int64_t)n_heads + 2 * (int64_t)n_kv_heads) * head_dim;
  p.slab = n_tokens * p.N;
  p.q = reinterpret_cast<uint16_t*>(q);
  p.k = reinterpret_cast<uint16_t*>(k);
  p.v = reinterpret_cast<uint16_t*>(v);
  p.qw = reinterpret_cast<const uint16_t*>(q_norm_weight);
  p.kw = reinterpret_cast<const uint16_t*>(k_norm_weight);
  p.positions = positions; p.cos_sin = cos_sin; p.slot_ids = slot_ids;
  p.kc = reinterpret_cast<uint16_t*>(key_cache);
  p.vc = reinterpret_cast<uint16_t*>(value_cache);
  p.q_ts = q_ts; p.k_ts = k_ts; p.v_ts = v_ts; p.T = n_tokens;
  p.eps = eps;
  p.n_splits = n_splits; p.interleaved = interleaved ? 1 : 0;
  p.n_heads = n_heads; p.n_kv_heads = n_kv_heads;
  p.head_tasks = (int)head_tasks; p.tasks_per_token = (int)tasks_per_token;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hip_clear_error();
  const dim3 g((unsigned)grid), blk(64 * kQkNormWaves);
  dispatch_dtype(dtype, [&](auto tag) {
    using TT = decltype(tag);
    auto by_dim = [&](auto cs_tag) {
      using CS = decltype(cs_tag);
      if (head_dim == 64) qk_norm_dispatch<TT, CS, 64>(p, slabs, g, blk, st);
      else if (head_dim == 128) qk_norm_dispatch<TT, CS, 128>(p, slabs, g, blk, st);
      else qk_norm_dispatch<TT, CS, 256>(p, slabs, g, blk, st);
    };
    if (cos_sin_is_f32) by_dim(float{});
    else by_dim(uint16_t{});
  });
  return hip_check_launch();
}

}  // namespace
}  // namespace slm

extern "C" SLM_API int slm_qk_norm_rope_kv_append(void* q, int64_t q_token_stride, void* k, int64_t k_token_stride,
                                                  const void* v, int64_t v_token_stride, const void* q_norm_weight,
                                                  const void* k_norm_weight, float eps, const int32_t* positions,
                                                  const void* cos_sin, int32_t cos_sin_is_f32, int32_t rot_dim,
                                                  int32_t interleaved, const int32_t* slot_ids, void* key_cache,
                                                  void* value_cache, int64_t n_tokens, int32_t n_heads,
                                                  int32_t n_kv_heads, int32_t head_dim, int32_t dtype, void* stream) {
  return slm::qk_norm_launch(nullptr, 0, q, q_token_stride, k, k_token_stride, const_cast<void*>(v), v_token_stride,
                             q_norm_weight, k_norm_weight, eps, positions, cos_sin, cos_sin_is_f32, rot_dim,
                             interleaved, slot_ids, key_cache, value_cache, n_tokens, n_heads, n_kv_heads, head_dim,
                             dtype, false, stream);
}

extern "C" SLM_API int slm_qk_norm_rope_kv_append_splitk(const float* partials, int32_t n_splits, void* q,
                                                         int64_t q_token_stride, void* k, int64_t k_token_stride,
                                                         void* v, int64_t v_token_stride, const void* q_norm_weight,
                                                         const void* k_norm_weight, float eps,
                                                         const int32_t* positions, const void* cos_sin,
                                                         int32_t cos_sin_is_f32, int32_t rot_dim, int32_t interleaved,
                                                         const int32_t* slot_ids, void* key_cache, void* value_cache,
                                                         int64_t n_tokens, int32_t n_heads, int32_t n_kv_heads,
                                                         int32_t head_dim, int32_t dtype, void* stream) {
  return slm::qk_norm_launch(partials, n_splits, q, q_token_stride, k, k_token_stride, v, v_token_stride,
                             q_norm_weight, k_norm_weight, eps, positions, cos_sin, cos_sin_is_f32, rot_dim,
                             interleaved, slot_ids, key_cache, value_cache, n_tokens, n_heads, n_kv_heads, head_dim,
                             dtype, true, stream);
}
