// gemma.hip -- what a Gemma / Gemma-2 layer needs beside the Llama glue (slm_hip.h section 12).
//
//  slm_gemma_norm  <- kernel::gemma_rms_norm (reference src/kernels/layernorm_kernels.cu:66-117; math
//                     src/layers/normalization.h:31-40: fp32 x * rsqrt(mean + eps) * (1 + w), ONE cast to T),
//                     the sandwich of src/models/google/gemma2.h:186-204 (post norm, residual add, pre norm of
//                     the sum) in one launch, reading the fp32 split-K slabs of a deferred o / down GEMM, and
//                     the scaled embedding of gemma2.h:236-238,270 with the first input norm.
//  slm_soft_cap    <- tanh(logits / cap) * cap (gemma2.h:341-342), one pass and one rounding.
#include "common.h"

namespace slm {

// GN(h, w) = T(h rs (1 + w)) on 8 values: fp32 throughout, the only rounding to T is the pack
template <typename T>
__device__ __forceinline__ u32x4 gemma_apply8(const float (&h)[8], const float rs, const u32x4 wv) {
  const float wf[8] = {lo_f32<T>(wv.x), hi_f32<T>(wv.x), lo_f32<T>(wv.y), hi_f32<T>(wv.y),
                       lo_f32<T>(wv.z), hi_f32<T>(wv.z), lo_f32<T>(wv.w), hi_f32<T>(wv.w)};
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = h[j] * rs * (1.0f + wf[j]);
  u32x4 r;
  r.x = pack2<T>(o[0], o[1]); r.y = pack2<T>(o[2], o[3]);
  r.z = pack2<T>(o[4], o[5]); r.w = pack2<T>(o[6], o[7]);
  return r;
}

// sum over the row of the four waves' partial sums; `red` is this reduction's own LDS slot
__device__ __forceinline__ float row_sum256(float v, float* red, const int tid) {
  v = group_sum<64>(v);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// One workgroup (256 threads) per token, NV vectors of 8 columns per thread, as rms_norm_kernel
// (glue.hip): the weights are issued first, every load is unconditional (vector index clamped, the
// contribution masked), the row stays in registers between the reductions.
//   form A  (residual == NULL):       out = GN(x, pre)
//   form B  (residual, table == NULL): y = GN(x, post) (post == NULL: y = x); residual = T(y + residual);
//                                      out = GN(residual, pre) when pre != NULL
//   form C  (table):                   residual = T(table[id] * x_scale); out = GN(residual, pre)
// x is a T row, or T(sum of the split-K slabs) rounded where the reduce kernel would have rounded.
template <typename T, int NV>
__global__ void __launch_bounds__(256) gemma_norm_kernel(
    uint16_t* out, const uint16_t* x /* may be out */, const float* __restrict__ part,
    const int n_splits, const int64_t slab, const uint16_t* __restrict__ post_w,
    const uint16_t* __restrict__ pre_w, uint16_t* __restrict__ residual,
    const uint16_t* __restrict__ table, const int* __restrict__ token_ids, const int64_t vocab,
    const float x_scale, const int64_t dim, const float eps) {
  __shared__ float red[2][4];
  const int64_t tok = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t nvec = dim / 8;
  const float inv_dim = 1.0f / (float)dim;
  u32x4 wpre[NV], wpost[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {  // the weights depend on nothing: issue them first
    const int64_t vic = min((int64_t)tid + 256 * i, nvec - 1);
    wpre[i] = pre_w ? *reinterpret_cast<const u32x4*>(pre_w + vic * 8) : u32x4{0u, 0u, 0u, 0u};
    wpost[i] = post_w ? *reinterpret_cast<const u32x4*>(post_w + vic * 8) : u32x4{0u, 0u, 0u, 0u};
  }
  const uint16_t* src = x + tok * dim;
  if (table) {  // an id outside the table must not become an address
    const int64_t id = min(max((int64_t)token_ids[tok], (int64_t)0), vocab - 1);
    src = table + id * dim;
  }
  u32x4 a[NV], r[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int64_t vic = min((int64_t)tid + 256 * i, nvec - 1);
    if (part) {  // x = T(sum of the split-K partial slabs): what the reduce kernel would have left
      const f32x4 s0 = splitk_sum4(part + tok * dim + vic * 8, slab, n_splits);
      const f32x4 s1 = splitk_sum4(part + tok * dim + vic * 8 + 4, slab, n_splits);
      a[i].x = pack2<T>(s0.x, s0.y); a[i].y = pack2<T>(s0.z, s0.w);
      a[i].z = pack2<T>(s1.x, s1.y); a[i].w = pack2<T>(s1.z, s1.w);
    } else {
      a[i] = *reinterpret_cast<const u32x4*>(src + vic * 8);
    }
    r[i] = (residual && !table) ? *reinterpret_cast<const u32x4*>(residual + tok * dim + vic * 8)
                                : u32x4{0u, 0u, 0u, 0u};
  }
  float v[NV][8];
#pragma unroll
  for (int i = 0; i < NV; ++i) unpack8<T>(a[i], v[i]);

  if (table) {  // form C: the product of two T values is exact in fp32, rounded once
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int64_t vi = tid + 256 * i;
      u32x4 w;
      w.x = pack2<T>(v[i][0] * x_scale, v[i][1] * x_scale); w.y = pack2<T>(v[i][2] * x_scale, v[i][3] * x_scale);
      w.z = pack2<T>(v[i][4] * x_scale, v[i][5] * x_scale); w.w = pack2<T>(v[i][6] * x_scale, v[i][7] * x_scale);
      if (vi < nvec) *reinterpret_cast<u32x4*>(residual + tok * dim + vi * 8) = w;
      unpack8<T>(w, v[i]);
    }
  } else if (residual) {  // form B
    float rs1 = 0.f;
    if (post_w) {
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if ((int64_t)tid + 256 * i < nvec) ss = rms_sumsq8(v[i], ss);
      rs1 = rsqrtf(row_sum256(ss, red[0], tid) * inv_dim + eps);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int64_t vi = tid + 256 * i;
      float y[8], rf[8];
      unpack8<T>(post_w ? gemma_apply8<T>(v[i], rs1, wpost[i]) : a[i], y);
      unpack8<T>(r[i], rf);
      u32x4 w;  // both addends are values of T: their fp32 sum rounds to T as the exact sum does
      w.x = pack2<T>(y[0] + rf[0], y[1] + rf[1]); w.y = pack2<T>(y[2] + rf[2], y[3] + rf[3]);
      w.z = pack2<T>(y[4] + rf[4], y[5] + rf[5]); w.w = pack2<T>(y[6] + rf[6], y[7] + rf[7]);
      if (vi < nvec) *reinterpret_cast<u32x4*>(residual + tok * dim + vi * 8) = w;
      unpack8<T>(w, v[i]);  // the second norm sees the ROUNDED sum, as a separate kernel would
    }
    if (!pre_w) return;
  }

  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if ((int64_t)tid + 256 * i < nvec) ss = rms_sumsq8(v[i], ss);
  const float rs = rsqrtf(row_sum256(ss, red[1], tid) * inv_dim + eps);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int64_t vi = tid + 256 * i;
    if (vi < nvec) *reinterpret_cast<u32x4*>(out + tok * dim + vi * 8) = gemma_apply8<T>(v[i], rs, wpre[i]);
  }
}

// tanh(z) in fp32, a few fp32 ulps of RELATIVE error at every magnitude (the result is rounded to T
// once, by the caller).  1 - 2 / (1 + e^{2z}) cancels for small z (below |z| ~ 1e-4 nothing of an f16
// result is left), so:
//   |z| <  0.25: the odd Taylor polynomial through z^9 (next term 0.0089 z^11: 8e-9 relative at 0.25)
//   |z| >= 0.25: (1 - e) / (1 + e), e = exp(-2 |z|) in (0, 0.61]: 1 - e >= 0.39 loses nothing, and
//                e underflows to 0 for large |z|, which gives exactly 1
__device__ __forceinline__ float tanh_f32(const float z) {
  const float az = __builtin_fabsf(z);
  const float z2 = z * z;
  float p = __builtin_fmaf(z2, 62.0f / 2835.0f, -17.0f / 315.0f);
  p = __builtin_fmaf(z2, p, 2.0f / 15.0f);
  p = __builtin_fmaf(z2, p, -1.0f / 3.0f);
  const float small = __builtin_fmaf(z * z2, p, z);
  const float e = fast_exp2(az * (-2.0f * 1.4426950408889634f));
  const float big = __builtin_copysignf((1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e), z);
  return az < 0.25f ? small : big;
}

// out = T(cap tanh(x / cap)) elementwise over n_rows * row_len / 8 vectors; out may be x (every thread
// reads its vector before it writes it)
template <typename T>
__global__ void __launch_bounds__(256) soft_cap_kernel(uint16_t* out, const uint16_t* x, const int64_t total,
                                                       const float cap, const float inv_cap) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const u32x4 g = *reinterpret_cast<const u32x4*>(x + idx * 8);
    float f[8];
    unpack8<T>(g, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = cap * tanh_f32(f[j] * inv_cap);
    u32x4 r;
    r.x = pack2<T>(f[0], f[1]); r.y = pack2<T>(f[2], f[3]);
    r.z = pack2<T>(f[4], f[5]); r.w = pack2<T>(f[6], f[7]);
    *reinterpret_cast<u32x4*>(out + idx * 8) = r;
  }
}

}  // namespace slm

using namespace slm;

extern "C" {

SLM_API int slm_gemma_norm(const slm_gemma_norm_args* a, void* stream) {
  if (!a || a->n_tokens < 0) return SLM_ERR_INVALID_ARG;
  if (a->n_tokens == 0) return SLM_OK;
  // the form is decided by the pointers; every combination outside the table of section 12 is an error
  const bool has_pre = a->pre_weight && a->out;
  if (a->table) {  // C
    if (!a->token_ids || !a->residual || !has_pre || a->x || a->partials || a->post_weight || a->vocab <= 0)
      return SLM_ERR_INVALID_ARG;
  } else if (a->residual) {  // B
    if (a->token_ids || (a->x != nullptr) == (a->partials != nullptr)) return SLM_ERR_INVALID_ARG;
    if ((a->pre_weight != nullptr) != (a->out != nullptr)) return SLM_ERR_INVALID_ARG;
    if (a->partials && a->n_splits < 1) return SLM_ERR_INVALID_ARG;
  } else {  // A
    if (!a->x || !has_pre || a->partials || a->post_weight || a->token_ids) return SLM_ERR_INVALID_ARG;
  }
  if (a->dtype != SLM_BF16 && a->dtype != SLM_F16) return SLM_ERR_UNSUPPORTED;
  if (a->dim <= 0 || a->dim % 8 || a->dim > 16384) return SLM_ERR_UNSUPPORTED;
  if (!aligned16(a->out) || !aligned16(a->x) || !aligned16(a->partials) || !aligned16(a->post_weight) ||
      !aligned16(a->pre_weight) || !aligned16(a->residual) || !aligned16(a->table) ||
      (reinterpret_cast<uintptr_t>(a->token_ids) & 3u))
    return SLM_ERR_ALIGNMENT;
  if (a->n_tokens > 0x7fffffffll) return SLM_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hip_clear_error();
  const dim3 grid((unsigned)a->n_tokens), blk(256);
  const int64_t slab = a->n_tokens * a->dim;
  const int64_t per_thread = (a->dim / 8 + 255) / 256;
#define SLM_GN(TT, NVV)                                                                              \
  hipLaunchKernelGGL((gemma_norm_kernel<TT, NVV>), grid, blk, 0, st, (uint16_t*)a->out,              \
                     (const uint16_t*)a->x, a->partials, (int)a->n_splits, slab,                     \
                     (const uint16_t*)a->post_weight, (const uint16_t*)a->pre_weight,                \
                     (uint16_t*)a->residual, (const uint16_t*)a->table, a->token_ids, a->vocab,      \
                     a->x_scale, a->dim, a->eps)
#define SLM_GN_NV(TT)                                                                                \
  do {                                                                                               \
    if (per_thread <= 1) SLM_GN(TT, 1); else if (per_thread <= 2) SLM_GN(TT, 2);                     \
    else if (per_thread <= 4) SLM_GN(TT, 4); else SLM_GN(TT, 8);                                     \
  } while (0)
  if (a->dtype == SLM_BF16) SLM_GN_NV(bf16_tag);
  else SLM_GN_NV(f16_tag);
#undef SLM_GN_NV
#undef SLM_GN
  return hip_check_launch();
}

SLM_API int slm_soft_cap(void* out, const void* x, int64_t n_rows, int64_t row_len, float cap, int32_t dtype,
                         void* stream) {
  if (n_rows == 0) return SLM_OK;
  if (!out || !x || n_rows < 0 || !(cap > 0.0f) || !(cap < 3.0e38f)) return SLM_ERR_INVALID_ARG;
  if (dtype != SLM_BF16 && dtype != SLM_F16) return SLM_ERR_UNSUPPORTED;
  if (row_len <= 0 || row_len % 8) return SLM_ERR_UNSUPPORTED;
  if (!aligned16(out) || !aligned16(x)) return SLM_ERR_ALIGNMENT;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hip_clear_error();
  const int64_t total = n_rows * (row_len / 8);
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  const dim3 grid((unsigned)blocks), blk(256);
  const float inv_cap = 1.0f / cap;
  if (dtype == SLM_BF16)
    hipLaunchKernelGGL(soft_cap_kernel<bf16_tag>, grid, blk, 0, st, (uint16_t*)out, (const uint16_t*)x, total, cap,
                       inv_cap);
  else
    hipLaunchKernelGGL(soft_cap_kernel<f16_tag>, grid, blk, 0, st, (uint16_t*)out, (const uint16_t*)x, total, cap,
                       inv_cap);
  return hip_check_launch();
}

}  // extern "C"
