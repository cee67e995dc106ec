// mla_glue.hip -- the MLA prologue (include/slm_hip.h section 18): what sits between the kv_a / q projection GEMM
// and slm_mla_paged_kv (section 11) in a DeepSeek-V2 layer, in ONE launch:
//   latent row  n = RMSNorm(c; w, eps) over the latent columns only        -> kv_cache[slot]
//   shared key  k_pe rotated by cos_sin[positions[t]]                       -> k_rope_cache[slot]
//   query tails q[t, h, nope:] rotated in place (plain form) / q written whole (slab form)
// The arithmetic is the existing kernels' own, shared through headers: rms_sumsq8 / rms_rstd / rms_apply8 and the
// wave64 reduction of rms_norm_kernel (common.h), rope_unit8 (rope.h), splitk_sum4 (common.h) -- so the results are
// bit-identical to slm_rms_norm, slm_rope_kv_append and the split-K reduce on the same values.
//
// Launch shape.  The rows are short (latent <= 512 = one 16-byte vector per lane of one wave; 64 rotary values per
// head = 8 lanes), so the unit of work is a WAVE TASK and nothing crosses a wave: no LDS, no barrier.  A token has
//   task 0:        the latent row -- lane i owns vector i exactly as thread i of rms_norm_kernel's first wave does,
//                  and the same butterfly adds the 64 partial sums, which is what makes the statistic bit-identical;
//   tasks 1 .. :   64 units each, first the (n_heads + 1) * 8 rotary units (heads, then the shared key), then in
//                  the slab form the n_heads * nope / 8 pass-through vectors of q.
// Four tasks share a 256-thread workgroup and tasks are numbered token-major, so one token (T = 1: 4 tasks with 16
// heads, 8 in the slab form) already fills one or two workgroups with independent waves, and a large T packs four
// rows' worth of waves per workgroup instead of launching a mostly idle 256-thread group per row.
#include "common.h"
#include "rope.h"

namespace slm {
namespace {

constexpr int kMlaGlueWaves = 4;
constexpr int kMlaRope = 64;  // section 11's rope_head_dim

struct MlaGlueParams {
  const float* part;  // slab form: [n_splits, T, N] fp32, else nullptr
  int64_t slab, N;
  uint16_t* q;
  const uint16_t* kv_a;
  const uint16_t* w;
  const int* positions;
  const void* cos_sin;
  const int* slot_ids;
  uint16_t* kvc;
  uint16_t* krc;
  int64_t q_ts, kva_ts, kvc_ss, krc_ss, T;
  float eps;
  int n_splits, interleaved, n_heads, nope, latent, tasks_per_token;
};

template <typename T, typename CS, bool PART>
__global__ void __launch_bounds__(64 * kMlaGlueWaves) mla_rope_append_kernel(const MlaGlueParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t task = (int64_t)blockIdx.x * kMlaGlueWaves + (threadIdx.x >> 6);
  const int64_t tok = task / p.tasks_per_token;
  if (tok >= p.T) return;  // wave-uniform; no barrier below
  const int sub = (int)(task - tok * p.tasks_per_token);
  const int64_t slot = (int64_t)p.slot_ids[tok];
  const int qk = p.nope + kMlaRope;
  const int64_t q_cols = (int64_t)p.n_heads * qk;  // slab row: [q heads | latent | k_pe]
  const float* prow = PART ? p.part + tok * p.N : nullptr;

  if (sub == 0) {  // ---- latent row: RMSNorm, to the cache slot
    const int nvec = p.latent / 8;
    const int vic = min(lane, nvec - 1);  // unconditional loads: index clamped, contribution masked
    const u32x4 wv = *reinterpret_cast<const u32x4*>(p.w + vic * 8);
    u32x4 a;
    if constexpr (PART) a = slab_sum8<T>(prow + q_cols + vic * 8, p.slab, p.n_splits);
    else a = *reinterpret_cast<const u32x4*>(p.kv_a + tok * p.kva_ts + vic * 8);
    float f[8];
    unpack8<T>(a, f);
    float ss = 0.f;
    if (lane < nvec) ss = rms_sumsq8(f, ss);
    ss = group_sum<64>(ss);
    const float rs = rms_rstd(ss, (float)p.latent, p.eps);
    if (lane < nvec && slot >= 0)
      *reinterpret_cast<u32x4*>(p.kvc + slot * p.kvc_ss + lane * 8) = rms_apply8<T>(f, rs, wv);
    return;
  }

  const int u = (sub - 1) * 64 + lane;
  const int rope_units = (p.n_heads + 1) * (kMlaRope / 8);
  if (u < rope_units) {  // ---- one 4 + 4-value rotary unit of a query head or of the shared key
    const int h = u >> 3, uu = u & 7;
    const bool is_k = h == p.n_heads;
    const int half = kMlaRope / 2;
    const int da = p.interleaved ? 8 * uu : 4 * uu, db = p.interleaved ? 8 * uu + 4 : half + 4 * uu;
    const CS* cs = reinterpret_cast<const CS*>(p.cos_sin) + (int64_t)p.positions[tok] * kMlaRope;
    float a[4], b[4], oa[4], ob[4];
    if constexpr (PART) {
      const float* src = prow + (is_k ? q_cols + p.latent : (int64_t)h * qk + p.nope);
      const f32x4 sa = splitk_sum4(src + da, p.slab, p.n_splits);
      const f32x4 sb = splitk_sum4(src + db, p.slab, p.n_splits);
      a[0] = lo_f32<T>((uint32_t)pack1<T>(sa.x)); a[1] = lo_f32<T>((uint32_t)pack1<T>(sa.y));
      a[2] = lo_f32<T>((uint32_t)pack1<T>(sa.z)); a[3] = lo_f32<T>((uint32_t)pack1<T>(sa.w));
      b[0] = lo_f32<T>((uint32_t)pack1<T>(sb.x)); b[1] = lo_f32<T>((uint32_t)pack1<T>(sb.y));
      b[2] = lo_f32<T>((uint32_t)pack1<T>(sb.z)); b[3] = lo_f32<T>((uint32_t)pack1<T>(sb.w));
    } else {
      const uint16_t* src = is_k ? p.kv_a + tok * p.kva_ts + p.latent : p.q + tok * p.q_ts + (int64_t)h * qk + p.nope;
      const u32x2 wa = *reinterpret_cast<const u32x2*>(src + da);  // adjacent under the interleaved pairing:
      const u32x2 wb = *reinterpret_cast<const u32x2*>(src + db);  // the two merge into one 16-byte load
      a[0] = lo_f32<T>(wa.x); a[1] = hi_f32<T>(wa.x); a[2] = lo_f32<T>(wa.y); a[3] = hi_f32<T>(wa.y);
      b[0] = lo_f32<T>(wb.x); b[1] = hi_f32<T>(wb.x); b[2] = lo_f32<T>(wb.y); b[3] = hi_f32<T>(wb.y);
    }
    rope_unit8<T>(a, b, cs, half, uu, p.interleaved, oa, ob);
    if (is_k && slot < 0) return;  // graph padding: the key has nowhere to go
    uint16_t* dst = is_k ? p.krc + slot * p.krc_ss : p.q + tok * p.q_ts + (int64_t)h * qk + p.nope;
    u32x2 ra, rb;
    ra.x = pack2<T>(oa[0], oa[1]); ra.y = pack2<T>(oa[2], oa[3]);
    rb.x = pack2<T>(ob[0], ob[1]); rb.y = pack2<T>(ob[2], ob[3]);
    *reinterpret_cast<u32x2*>(dst + da) = ra;
    *reinterpret_cast<u32x2*>(dst + db) = rb;
    return;
  }
  if constexpr (PART) {  // ---- the nope columns of q: T(sum), 8 columns per lane
    const int vph = p.nope / 8;  // vectors per head
    const int i = u - rope_units;
    if (i >= p.n_heads * vph) return;
    const int h = i / vph, c = (i - h * vph) * 8;
    const u32x4 a = slab_sum8<T>(prow + (int64_t)h * qk + c, p.slab, p.n_splits);
    *reinterpret_cast<u32x4*>(p.q + tok * p.q_ts + (int64_t)h * qk + c) = a;
  }
}

inline bool stride16(int64_t elems) { return (elems & 7) == 0; }

int mla_rope_append_launch(const float* partials, int32_t n_splits, void* q, int64_t q_ts, const void* kv_a,
                           int64_t kva_ts, const void* weight, float eps, const int32_t* positions,
                           const void* cos_sin, int32_t cos_sin_is_f32, int32_t interleaved, const int32_t* slot_ids,
                           void* kv_cache, void* k_rope_cache, int64_t kvc_ss, int64_t krc_ss, int64_t n_tokens,
                           int32_t n_heads, int32_t nope, int32_t latent, int32_t rope, int32_t dtype, bool slabs,
                           void* stream) {
  if (n_tokens < 0 || n_tokens > 0x7fffffffLL || n_heads < 0 || nope < 0 || latent <= 0 || rope <= 0)
    return SLM_ERR_INVALID_ARG;
  if (n_tokens == 0) return SLM_OK;
  if ((slabs ? !partials || n_splits < 1 : !kv_a) || !weight || !positions || !cos_sin || !slot_ids || !kv_cache ||
      !k_rope_cache || (n_heads > 0 && !q))
    return SLM_ERR_INVALID_ARG;
  if (dtype != SLM_F16 && dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if ((latent != 128 && latent != 256 && latent != 512) || rope != kMlaRope || nope % 8) return SLM_ERR_UNSUPPORTED;
  if (!aligned16(partials) || !aligned16(q) || !aligned16(kv_a) || !aligned16(weight) || !aligned16(cos_sin) ||
      !aligned16(kv_cache) || !aligned16(k_rope_cache) || !stride16(kvc_ss) || !stride16(krc_ss) ||
      (n_heads > 0 && !stride16(q_ts)) || (!slabs && !stride16(kva_ts)))
    return SLM_ERR_ALIGNMENT;
  const int64_t units = (int64_t)(n_heads + 1) * (kMlaRope / 8) + (slabs ? (int64_t)n_heads * (nope / 8) : 0);
  const int64_t tasks_per_token = 1 + (units + 63) / 64;
  const int64_t grid = (n_tokens * tasks_per_token + kMlaGlueWaves - 1) / kMlaGlueWaves;
  if (tasks_per_token > 0x7fffffffLL || grid > 0x7fffffffLL) return SLM_ERR_UNSUPPORTED;
  MlaGlueParams p;
  p.part = slabs ? partials : nullptr;
  p.N = (int64_t)n_heads * (nope + kMlaRope) + latent + kMlaRope;
  p.slab = n_tokens * p.N;
  p.q = reinterpret_cast<uint16_t*>(q);
  p.kv_a = reinterpret_cast<const uint16_t*>(kv_a);
  p.w = reinterpret_cast<const uint16_t*>(weight);
  p.positions = positions; p.cos_sin = cos_sin; p.slot_ids = slot_ids;
  p.kvc = reinterpret_cast<uint16_t*>(kv_cache);
  p.krc = reinterpret_cast<uint16_t*>(k_rope_cache);
  p.q_ts = q_ts; p.kva_ts = kva_ts; p.kvc_ss = kvc_ss; p.krc_ss = krc_ss; p.T = n_tokens;
  p.eps = eps;
  p.n_splits = n_splits; p.interleaved = interleaved ? 1 : 0;
  p.n_heads = n_heads; p.nope = nope; p.latent = latent; p.tasks_per_token = (int)tasks_per_token;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hip_clear_error();
  const dim3 g((unsigned)grid), blk(64 * kMlaGlueWaves);
  dispatch_dtype(dtype, [&](auto tag) {
    using TT = decltype(tag);
    if (slabs) {
      if (cos_sin_is_f32) hipLaunchKernelGGL((mla_rope_append_kernel<TT, float, true>), g, blk, 0, st, p);
      else hipLaunchKernelGGL((mla_rope_append_kernel<TT, uint16_t, true>), g, blk, 0, st, p);
    } else {
      if (cos_sin_is_f32) hipLaunchKernelGGL((mla_rope_append_kernel<TT, float, false>), g, blk, 0, st, p);
      else hipLaunchKernelGGL((mla_rope_append_kernel<TT, uint16_t, false>), g, blk, 0, st, p);
    }
  });
  return hip_check_launch();
}

}  // namespace
}  // namespace slm

extern "C" SLM_API int slm_mla_rope_append(void* q, int64_t q_token_stride, const void* kv_a,
                                           int64_t kv_a_token_stride, const void* norm_weight, float eps,
                                           const int32_t* positions, const void* cos_sin, int32_t cos_sin_is_f32,
                                           int32_t interleaved, const int32_t* slot_ids, void* kv_cache,
                                           void* k_rope_cache, int64_t kv_slot_stride, int64_t k_rope_slot_stride,
                                           int64_t n_tokens, int32_t n_heads, int32_t nope_head_dim,
                                           int32_t latent_dim, int32_t rope_head_dim, int32_t dtype, void* stream) {
  return slm::mla_rope_append_launch(nullptr, 0, q, q_token_stride, kv_a, kv_a_token_stride, norm_weight, eps,
                                     positions, cos_sin, cos_sin_is_f32, interleaved, slot_ids, kv_cache,
                                     k_rope_cache, kv_slot_stride, k_rope_slot_stride, n_tokens, n_heads,
                                     nope_head_dim, latent_dim, rope_head_dim, dtype, false, stream);
}

extern "C" SLM_API int slm_mla_rope_append_splitk(const float* partials, int32_t n_splits, void* q,
                                                  int64_t q_token_stride, const void* norm_weight, float eps,
                                                  const int32_t* positions, const void* cos_sin,
                                                  int32_t cos_sin_is_f32, int32_t interleaved,
                                                  const int32_t* slot_ids, void* kv_cache, void* k_rope_cache,
                                                  int64_t kv_slot_stride, int64_t k_rope_slot_stride,
                                                  int64_t n_tokens, int32_t n_heads, int32_t nope_head_dim,
                                                  int32_t latent_dim, int32_t rope_head_dim, int32_t dtype,
                                                  void* stream) {
  return slm::mla_rope_append_launch(partials, n_splits, q, q_token_stride, nullptr, 0, norm_weight, eps, positions,
                                     cos_sin, cos_sin_is_f32, interleaved, slot_ids, kv_cache, k_rope_cache,
                                     kv_slot_stride, k_rope_slot_stride, n_tokens, n_heads, nope_head_dim,
                                     latent_dim, rope_head_dim, dtype, true, stream);
}
