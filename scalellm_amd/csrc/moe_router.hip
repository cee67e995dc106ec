// moe_router.hip -- the fused MoE router (include/slm_hip.h section 17, slm_moe_router): the gate GEMM
//     logit[t, e] = sum_h x[t, h] * gate_w[e, h]        (fp32 MFMA accumulation, never rounded to T)
// and section 10's routing of those logits, in ONE launch.
//
// One workgroup (4 waves) owns a tile of 32 token rows and all E columns.  x rows are the A operand and gate rows
// the B operand of the 32x32x16 MFMA, and both are k-contiguous in memory: lane (r = lane & 31, h = lane >> 5) holds
// 8 consecutive k of row r, so both go from global memory to the MFMA in 16-B loads -- no LDS stage, no transpose,
// no fp32 copy of the gate (moe_gemm.hip feeds W the same way).  K is walked in 128-deep chunks, lane half h taking
// the 128 contiguous bytes [128 h, 128 h + 128) of the chunk's 256 B of a row, then in up to three 32-deep units.
//
// Work split.  ES = max(E, 32) columns are ES / 32 column tiles.  With 4 or 8 tiles every wave owns 1 or 2 column
// tiles over the whole K; with 2 tiles the waves are 2 tiles x 2 K slices, with 1 tile 4 K slices.  A slice is a
// range of 32-deep units computed from hidden alone.  The K partials meet in LDS and are added in slice order
// 0, 1, 2, 3.  So what is added to what, and in which order, is a function of (hidden, E, dtype) -- never of T, of
// the row's index or of the other rows in the tile: a row routed alone gives the bits it gives in any batch.
//
// Then wave w routes rows w, w + 4, ... of the tile with moe_route.h's per-token routines on the LDS logits -- the
// code slm_moe_topk_softmax / slm_moe_grouped_topk_sigmoid run, hence their bits.
//
// Tile edges: rows >= T load row T - 1 and gate rows >= E load row E - 1; neither is ever stored.
// No workspace, no atomics, no workgroup waits for another.
#include "common.h"
#include "moe_route.h"

namespace slm {
namespace {

constexpr int kRtRows = 32;                 // token rows per workgroup
constexpr int kRtWaves = kRouteWaves;       // 4: GroupedSmem has one row per wave
constexpr int kRtThreads = 64 * kRtWaves;

struct RouterKParams {
  const char* x;
  const char* w;
  const float* bias;
  float* weights;
  int* indices;
  float* logits_out;
  int64_t T;
  int64_t ldx, ldw;  // elements
  int n_units;       // hidden / 32
  int E, k;
  int scoring, renorm, n_groups, topk_group;
  float scaling;
};

// TPW: column tiles per wave (2 when E = 256)
template <typename T, int TPW>
__global__ void __launch_bounds__(kRtThreads) moe_router_kernel(const RouterKParams p) {
  typedef typename Mfma<T>::frag frag_t;
  __shared__ float s_logit[kRtRows * kMaxRouteExperts];  // [k slice][32][ES] partials, then [32][ES] logits
  __shared__ GroupedSmem s_grp;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int E = p.E;
  const int ES = E < 32 ? 32 : E;
  const int nct = ES >> 5;                    // 1, 2, 4, 8
  const int cw = nct < 4 ? nct : 4;           // waves side by side on column tiles
  const int ksplit = kRtWaves / cw;           // K slices: 4, 2, 1, 1
  const int ct0 = wave % cw, ks = wave / cw;
  const int64_t t0 = (int64_t)blockIdx.x * kRtRows;
  const int mrow = lane & 31, kh = lane >> 5;

  // ---- the gate GEMM of this wave: column tiles ct0 (+ cw j), units [u0, u1) ----
  const int u0 = (int)((int64_t)p.n_units * ks / ksplit), u1 = (int)((int64_t)p.n_units * (ks + 1) / ksplit);
  int64_t xr = t0 + mrow;
  if (xr >= p.T) xr = p.T - 1;  // clamped, never stored
  const char* arow = p.x + 2 * (xr * p.ldx) + (int64_t)u0 * 64;
  const char* brow[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    int er = (ct0 + cw * j) * 32 + mrow;
    if (er >= E) er = E - 1;    // the masked column tile of E < 32
    brow[j] = p.w + 2 * ((int64_t)er * p.ldw) + (int64_t)u0 * 64;
  }
  f32x16 acc[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int nC = (u1 - u0) >> 2;  // 128-deep chunks
  if (nC > 0) {
    const int last = nC - 1;
    u32x4 a[2][8], b[2][TPW][8];
    auto load = [&](int c, u32x4 (&av)[8], u32x4 (&bv)[TPW][8]) {
      const int64_t off = (int64_t)(c < last ? c : last) * 256 + kh * 128;  // past the end: the last chunk again
#pragma unroll
      for (int q = 0; q < 8; ++q) av[q] = *reinterpret_cast<const u32x4*>(arow + off + q * 16);
#pragma unroll
      for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int q = 0; q < 8; ++q) bv[j][q] = *reinterpret_cast<const u32x4*>(brow[j] + off + q * 16);
    };
    auto mma = [&](const u32x4 (&av)[8], const u32x4 (&bv)[TPW][8]) {
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int j = 0; j < TPW; ++j)
          acc[j] = Mfma<T>::run(__builtin_bit_cast(frag_t, av[q]), __builtin_bit_cast(frag_t, bv[j][q]), acc[j]);
    };
    load(0, a[0], b[0]);
    for (int c = 0; c < nC; c += 2) {  // chunk c in set 0, c + 1 in set 1: the next loads fly over the MFMAs
      load(c + 1, a[1], b[1]);
      mma(a[0], b[0]);
      load(c + 2, a[0], b[0]);
      if (c + 1 < nC) mma(a[1], b[1]);
    }
  }
  // up to three 32-deep units: lane half kh holds k = 16 kh + 8 s + j of the unit
  for (int u = u0 + 4 * nC; u < u1; ++u) {
    const int64_t off = (int64_t)(u - u0) * 64 + kh * 32;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const u32x4 av = *reinterpret_cast<const u32x4*>(arow + off + s * 16);
#pragma unroll
      for (int j = 0; j < TPW; ++j) {
        const u32x4 bv = *reinterpret_cast<const u32x4*>(brow[j] + off + s * 16);
        acc[j] = Mfma<T>::run(__builtin_bit_cast(frag_t, av), __builtin_bit_cast(frag_t, bv), acc[j]);
      }
    }
  }

  // ---- partials to LDS: C/D layout col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) ----
  const int slab = kRtRows * ES;  // <= 8192 floats; ksplit * slab <= 8192 as well
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    float* dst = s_logit + ks * slab + (ct0 + cw * j) * 32 + mrow;
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[((r & 3) + 8 * (r >> 2) + 4 * kh) * ES] = acc[j][r];
  }
  __syncthreads();
  // slices added in order 0, 1, 2, 3 into slab 0; the logits leave from here as well
  const int es_shift = 31 - __builtin_clz(ES);
  for (int i = tid; i < slab; i += kRtThreads) {
    float v = s_logit[i];
    for (int s = 1; s < ksplit; ++s) v += s_logit[s * slab + i];
    if (ksplit > 1) s_logit[i] = v;
    const int r = i >> es_shift, e = i & (ES - 1);
    if (p.logits_out && t0 + r < p.T && e < E) p.logits_out[(t0 + r) * E + e] = v;
  }
  __syncthreads();

  // ---- routing: wave w takes rows w, w + 4, ...; every wave makes every trip (the grouped form has barriers) ----
  const int k = p.k;
  for (int r = wave; r < kRtRows; r += kRtWaves) {
    const int64_t t = t0 + r;
    const bool live = t < p.T;
    if (p.scoring == 0) {
      if (live) route_topk_softmax_wave(s_logit + r * ES, p.weights + t * k, p.indices + t * k, lane, E, k, p.renorm);
    } else {
      // a row beyond T: its clamped copy of row T - 1, routed and never stored
      const int64_t tt = live ? t : 0;
      route_grouped_sigmoid_wave(s_logit + r * ES, p.bias, s_grp, wave, p.weights + tt * k, p.indices + tt * k, live,
                                 lane, E, p.n_groups, p.topk_group, k, p.scaling);
    }
  }
}

template <typename T>
void launch_router(const RouterKParams& kp, unsigned grid, hipStream_t st) {
  if (kp.E > 128) hipLaunchKernelGGL((moe_router_kernel<T, 2>), dim3(grid), dim3(kRtThreads), 0, st, kp);
  else hipLaunchKernelGGL((moe_router_kernel<T, 1>), dim3(grid), dim3(kRtThreads), 0, st, kp);
}

int router_shape_check(int32_t E, int64_t hidden, int32_t dtype) {
  if (E < 1 || hidden < 1) return SLM_ERR_INVALID_ARG;
  if (dtype != SLM_F16 && dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (!is_pow2(E) || E > kMaxRouteExperts || hidden % 32 || hidden >= ((int64_t)1 << 31)) return SLM_ERR_UNSUPPORTED;
  return SLM_OK;
}

}  // namespace
}  // namespace slm

extern "C" {

SLM_API int slm_moe_router_splits(int32_t n_experts, int64_t hidden, int32_t dtype, int32_t* splits) {
  const int rc = slm::router_shape_check(n_experts, hidden, dtype);
  if (rc != SLM_OK) return rc;
  if (!splits) return SLM_ERR_INVALID_ARG;
  *splits = 1;  // one workgroup per row tile over the whole K
  return SLM_OK;
}

SLM_API int slm_moe_router_workspace_bytes(int64_t n_tokens, int32_t n_experts, int64_t hidden, int32_t dtype,
                                           size_t* bytes) {
  if (n_tokens < 0) return SLM_ERR_INVALID_ARG;
  int32_t splits = 0;
  const int rc = slm_moe_router_splits(n_experts, hidden, dtype, &splits);
  if (rc != SLM_OK) return rc;
  if (!bytes) return SLM_ERR_INVALID_ARG;
  *bytes = 0;  // splits == 1: the partials never leave the workgroup
  return SLM_OK;
}

SLM_API int slm_moe_router(const slm_moe_router_args* a, void* stream) {
  using namespace slm;
  if (!a) return SLM_ERR_INVALID_ARG;
  if (a->n_tokens < 0 || a->hidden < 1 || a->n_experts < 1 || a->workspace_bytes < 0) return SLM_ERR_INVALID_ARG;
  if (a->scoring != 0 && a->scoring != 1) return SLM_ERR_INVALID_ARG;
  int rc = route_shape_check(a->n_tokens, a->n_experts, a->topk);
  if (rc == SLM_OK) rc = router_shape_check(a->n_experts, a->hidden, a->dtype);
  if (rc != SLM_OK) return rc;
  if (a->scoring == 1 &&
      route_groups_check(a->n_experts, a->n_expert_groups, a->topk_group, a->topk) != SLM_OK)
    return SLM_ERR_INVALID_ARG;
  if (a->n_tokens == 0) return SLM_OK;
  if (!a->x || !a->gate_w || !a->weights || !a->indices) return SLM_ERR_INVALID_ARG;
  if (a->scoring == 1 && !a->correction_bias) return SLM_ERR_INVALID_ARG;
  if (a->ldx < a->hidden || a->ldw < a->hidden) return SLM_ERR_INVALID_ARG;
  if (!aligned16(a->x) || !aligned16(a->gate_w) || a->ldx % 8 || a->ldw % 8 ||
      (reinterpret_cast<uintptr_t>(a->weights) & 3u) || (reinterpret_cast<uintptr_t>(a->indices) & 3u) ||
      (reinterpret_cast<uintptr_t>(a->logits_out) & 3u) || (reinterpret_cast<uintptr_t>(a->correction_bias) & 3u))
    return SLM_ERR_ALIGNMENT;
  size_t need = 0;
  (void)slm_moe_router_workspace_bytes(a->n_tokens, a->n_experts, a->hidden, a->dtype, &need);
  if (need > 0 && (!a->workspace || (uint64_t)a->workspace_bytes < need)) return SLM_ERR_WORKSPACE;
  const int64_t grid = (a->n_tokens + kRtRows - 1) / kRtRows;
  if (grid >= ((int64_t)1 << 31)) return SLM_ERR_UNSUPPORTED;

  RouterKParams kp;
  kp.x = reinterpret_cast<const char*>(a->x);
  kp.w = reinterpret_cast<const char*>(a->gate_w);
  kp.bias = a->correction_bias;
  kp.weights = a->weights;
  kp.indices = a->indices;
  kp.logits_out = a->logits_out;
  kp.T = a->n_tokens;
  kp.ldx = a->ldx; kp.ldw = a->ldw;
  kp.n_units = (int)(a->hidden / 32);
  kp.E = a->n_experts; kp.k = a->topk;
  kp.scoring = a->scoring; kp.renorm = a->renormalize;
  kp.n_groups = a->n_expert_groups; kp.topk_group = a->topk_group;
  kp.scaling = a->scaling_factor;
  hip_clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dispatch_dtype(a->dtype, [&](auto t) { launch_router<decltype(t)>(kp, (unsigned)grid, st); });
  return hip_check_launch();
}

}  // extern "C"
