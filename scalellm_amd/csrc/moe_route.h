// moe_route.h -- THE per-token routing code of include/slm_hip.h section 10, one wave per token.  Shared by the
// routing kernels over fp32 logits in global memory (moe.hip) and by the fused router, which runs it on the logits
// its gate GEMM left in LDS (moe_router.hip): one code, so the two give identical bits on identical logits.
#pragma once
#include <math.h>

#include "common.h"

namespace slm {

constexpr int kMaxRouteExperts = 256;  // the reference's own limit for both routing kernels
constexpr int kRouteWaves = 4;         // tokens (waves) per routing workgroup
constexpr int kEpl = kMaxRouteExperts / 64;  // experts per lane: lane l holds l, l + 64, ...
constexpr int kNoIdx = 0x7fffffff;

// (value, index) candidates: higher value first, then the lower index (-0 == +0: a tie)
__device__ __forceinline__ bool ranks_before(float v, int i, float w, int j) {
  return v > w || (v == w && i < j);
}

// the best remaining candidate of the wave's E values: every lane returns the same (v, idx)
__device__ __forceinline__ void wave_best(const float (&val)[kEpl], const unsigned taken, const int lane,
                                          const int E, float& bv, int& bi) {
  bv = -INFINITY;
  bi = kNoIdx;
#pragma unroll
  for (int s = 0; s < kEpl; ++s) {
    const int e = lane + 64 * s;
    if (e < E && !((taken >> s) & 1u) && ranks_before(val[s], e, bv, bi)) { bv = val[s]; bi = e; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ranks_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
// butterfly sum: every lane adds the same pairs in the same order
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// top-k of the softmax of one token: x = its E logits, w_out / i_out = its k outputs.  No workgroup barrier.
__device__ __forceinline__ void route_topk_softmax_wave(const float* x, float* w_out, int* i_out, const int lane,
                                                        const int E, const int k, const int renorm) {
  float val[kEpl];
  float m = -INFINITY;
#pragma unroll
  for (int s = 0; s < kEpl; ++s) {
    const int e = lane + 64 * s;
    val[s] = e < E ? x[e] : -INFINITY;
    m = fmaxf(m, val[s]);
  }
  m = wave_max(m);
  float sum = 0.f;
#pragma unroll
  for (int s = 0; s < kEpl; ++s)
    if (lane + 64 * s < E) sum += expf(val[s] - m);
  sum = wave_sum(sum);

  // lane j & 63 keeps output j (slot j >> 6) until the sum of the k weights is known
  float pj[kEpl] = {};
  int ij[kEpl] = {};
  unsigned taken = 0;
  float wsum = 0.f;
  for (int j = 0; j < k; ++j) {
    float bv;
    int bi;
    wave_best(val, taken, lane, E, bv, bi);
    if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
    const float p = expf(bv - m) / sum;
    wsum += p;  // in order j = 0 .. k - 1, the same in every lane
    if ((j & 63) == lane) {
#pragma unroll
      for (int s = 0; s < kEpl; ++s)
        if ((j >> 6) == s) { pj[s] = p; ij[s] = bi; }
    }
  }
#pragma unroll
  for (int s = 0; s < kEpl; ++s) {
    const int j = lane + 64 * s;
    if (j < k) {
      w_out[j] = renorm ? pj[s] / wsum : pj[s];
      i_out[j] = ij[s];
    }
  }
}

// the wave's own LDS rows of the grouped routing
struct GroupedSmem {
  float c[kRouteWaves][kMaxRouteExperts];      // biased scores
  float gscore[kRouteWaves][kMaxRouteExperts / 2];
  int gkeep[kRouteWaves][kMaxRouteExperts / 2];
};

// group-limited top-k of the biased sigmoid scores of one token (wave wv of the workgroup).  It holds three
// workgroup barriers: EVERY wave of the workgroup calls it the same number of times; a wave without a token of its
// own passes live = false with a valid x (duplicate work, never stored).
__device__ __forceinline__ void route_grouped_sigmoid_wave(const float* x, const float* __restrict__ bias,
                                                           GroupedSmem& sm, const int wv, float* w_out, int* i_out,
                                                           const bool live, const int lane, const int E,
                                                           const int n_groups, const int topk_group, const int k,
                                                           const float scaling) {
  const int gsz = E / n_groups;
  float s[kEpl], val[kEpl];
#pragma unroll
  for (int q = 0; q < kEpl; ++q) {
    const int e = lane + 64 * q;
    s[q] = 0.f;
    val[q] = -INFINITY;
    if (e < E) {
      s[q] = 1.0f / (1.0f + expf(-x[e]));
      val[q] = s[q] + bias[e];
      sm.c[wv][e] = val[q];
    }
  }
  __syncthreads();
  // group score: the sum of the group's two largest biased scores
  for (int g = lane; g < n_groups; g += 64) {
    float a = -INFINITY, b = -INFINITY;  // a >= b
    for (int i = 0; i < gsz; ++i) {
      const float v = sm.c[wv][g * gsz + i];
      if (v > a) { b = a; a = v; }
      else if (v > b) b = v;
    }
    sm.gscore[wv][g] = a + b;
  }
  __syncthreads();
  // a group is kept when fewer than topk_group groups rank before it (ties: the lower group first)
  for (int g = lane; g < n_groups; g += 64) {
    const float me = sm.gscore[wv][g];
    int before = 0;
    for (int h = 0; h < n_groups; ++h) before += ranks_before(sm.gscore[wv][h], h, me, g) ? 1 : 0;
    sm.gkeep[wv][g] = before < topk_group ? 1 : 0;
  }
  __syncthreads();
  unsigned taken = 0;
#pragma unroll
  for (int q = 0; q < kEpl; ++q) {
    const int e = lane + 64 * q;
    if (e >= E || !sm.gkeep[wv][e / gsz]) taken |= 1u << q;  // masked out: never a candidate
  }
  for (int j = 0; j < k; ++j) {
    float bv;
    int bi;
    wave_best(val, taken, lane, E, bv, bi);
    if (bi == kNoIdx) break;  // k <= kept experts is checked on the host
    if ((bi & 63) == lane) {
      taken |= 1u << (bi >> 6);
      if (live) {
        float sv = 0.f;
#pragma unroll
        for (int q = 0; q < kEpl; ++q)
          if ((bi >> 6) == q) sv = s[q];
        w_out[j] = sv * scaling;
        i_out[j] = bi;
      }
    }
  }
}

// the argument rules both routing entries and the fused router share
inline int route_shape_check(int64_t T, int32_t E, int32_t k) {
  if (T < 0 || E < 1 || k < 1 || k > E) return SLM_ERR_INVALID_ARG;
  if (!is_pow2(E) || E > kMaxRouteExperts) return SLM_ERR_UNSUPPORTED;
  return SLM_OK;
}
inline int route_groups_check(int32_t E, int32_t n_groups, int32_t topk_group, int32_t k) {
  if (n_groups < 1 || E % n_groups || E / n_groups < 2 || topk_group < 1 || topk_group > n_groups ||
      (int64_t)k > (int64_t)topk_group * (E / n_groups))
    return SLM_ERR_INVALID_ARG;
  return SLM_OK;
}

}  // namespace slm
