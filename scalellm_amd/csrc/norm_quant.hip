// norm_quant.hip -- RMSNorm that writes the next GEMM's MXFP4 input (include/slm_hip.h section 24):
//   slm_rms_norm_mxfp4 / slm_rms_norm_mxfp4_splitk: x (or the split-K slabs) [+ residual] -> aq [T, dim/2] e2m1 codes +
//   a_scale [T, dim/32] e8m0 bytes (+ the T row on request): byte for byte slm_w4a4_quantize_act run on slm_rms_norm's
//   (slm_rms_norm_splitk's) output, one launch and one round trip of the normalised row less.
//
// The arithmetic is the two kernels' own, shared through headers: rms_sumsq8 / rms_rstd / rms_apply8 / splitk_sum4 and
// the reduction order of rms_norm_kernel (common.h; glue.hip), act_amax_pk / act_amax15 / act_block_e8m0 /
// act_cvt_scale / act_cvt8 of the quantiser (w4a4_quant.h).
//
// Split.  rms_norm_kernel's: one workgroup (256 threads) per token, thread tid owns the 8 columns of vector
// tid + 256 i, i < NV = 1 / 2 / 4 / 8.  An MX block (32 columns) is then the four lanes of a quad, and dim % 32 == 0
// puts a quad wholly inside or wholly outside the row.  After rms_apply8 a lane holds its 8 values as four dwords of T:
//   amax    packed-u16 maxima over the four dwords, then two DPP quad_perm exchanges -- every lane of the quad holds the
//           block's amax and derives the same e8m0 byte; no LDS, no barrier beyond the norm's own
//   codes   act_cvt8: the lane's 8 values -> ONE dword; lane 0 of the quad collects the other three (DPP row_shl 1, 2, 3)
//           and stores the block's 16 bytes at once
//   scales  a row of 16 lanes is four neighbouring blocks: lane 0 collects the four bytes (DPP row_shl 4, 8, 12) and
//           stores one dword where the token's scale row is 4-byte aligned and all four blocks exist; otherwise each
//           quad's lane 0 stores its byte (ldas carries no alignment, and bytes past dim / 32 are never written)
// All cross-lane steps run in every lane (vector indices are clamped as in rms_norm_kernel); only the stores are masked.
// Compiled with glue.hip's flags (no file flags of its own).
#include "common.h"
#include "w4a4_quant.h"

namespace slm {

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
constexpr int DPP_ROW_SHL = 0x100;  // + n: lane l reads lane l + n of its row of 16 (0 past the row's end)

template <typename T, int NV>
__global__ void __launch_bounds__(256) rms_norm_mxfp4_kernel(char* __restrict__ aq, int64_t ldaq,
                                                             uint8_t* __restrict__ a_scale, int64_t ldas,
                                                             uint16_t* __restrict__ out, const uint16_t* __restrict__ x,
                                                             const uint16_t* __restrict__ weight,
                                                             uint16_t* __restrict__ residual, int64_t dim, float eps,
                                                             const float* __restrict__ part, int n_splits, int64_t slab) {
  __shared__ float red[4];
  const int64_t tok = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t nvec = dim / 8;
  float v[NV][8];
  u32x4 wv[NV];
  float ss = 0.f;
  // ---- the row, the residual update and the sum of squares: rms_norm_kernel's steps in its order ----
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int64_t vic = min((int64_t)tid + 256 * i, nvec - 1);
    wv[i] = *reinterpret_cast<const u32x4*>(weight + vic * 8);
  }
  u32x4 a[NV], r[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int64_t vic = min((int64_t)tid + 256 * i, nvec - 1);
    if (part) a[i] = slab_sum8<T>(part + tok * dim + vic * 8, slab, n_splits);
    else a[i] = *reinterpret_cast<const u32x4*>(x + tok * dim + vic * 8);
    r[i] = residual ? *reinterpret_cast<const u32x4*>(residual + tok * dim + vic * 8) : u32x4{0u, 0u, 0u, 0u};
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int64_t vi = tid + 256 * i;
    const bool valid = vi < nvec;
    float f[8];
    unpack8<T>(a[i], f);
    if (residual) {
      float g[8];
      unpack8<T>(r[i], g);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += g[j];
      u32x4 w;
      w.x = pack2<T>(f[0], f[1]); w.y = pack2<T>(f[2], f[3]);
      w.z = pack2<T>(f[4], f[5]); w.w = pack2<T>(f[6], f[7]);
      if (valid) *reinterpret_cast<u32x4*>(residual + tok * dim + vi * 8) = w;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[i][j] = f[j];
    if (valid) ss = rms_sumsq8(f, ss);
  }
  ss = group_sum<64>(ss);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  const float tot = red[0] + red[1] + red[2] + red[3];
  const float rs = rms_rstd(tot, (float)dim, eps);

  // ---- normalise, quantise the quad's block, store ----
  char* qrow = aq + tok * ldaq;
  uint8_t* srow = a_scale + tok * ldas;
  const bool srow4 = (reinterpret_cast<uintptr_t>(srow) & 3u) == 0;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int64_t vi = tid + 256 * i;
    const bool valid = vi < nvec;
    const u32x4 o = rms_apply8<T>(v[i], rs, wv[i]);
    if (out && valid) *reinterpret_cast<u32x4*>(out + tok * dim + vi * 8) = o;
    uint32_t mx = act_amax_pk(0u, o);
    mx = pk_max_u16(mx, dpp_u32<DPP_QUAD_XOR1>(mx));
    mx = pk_max_u16(mx, dpp_u32<DPP_QUAD_XOR2>(mx));
    const uint32_t e8 = act_block_e8m0<T>(act_amax15(mx));
    const uint32_t d = act_cvt8<T>(o, act_cvt_scale(e8));
    const u32x4 codes = {d, dpp_u32<DPP_ROW_SHL + 1>(d), dpp_u32<DPP_ROW_SHL + 2>(d), dpp_u32<DPP_ROW_SHL + 3>(d)};
    const uint32_t e4 = e8 | dpp_u32<DPP_ROW_SHL + 4>(e8) << 8 | dpp_u32<DPP_ROW_SHL + 8>(e8) << 16 |
                        dpp_u32<DPP_ROW_SHL + 12>(e8) << 24;
    if (valid && (tid & 3) == 0) {
      const int64_t blk = vi >> 2;
      *reinterpret_cast<u32x4*>(qrow + blk * 16) = codes;
      if (srow4 && (vi | 15) < nvec) {  // the four blocks of this row of lanes exist: one dword from its lane 0
        if ((tid & 15) == 0) *reinterpret_cast<uint32_t*>(srow + blk) = e4;
      } else {
        srow[blk] = (uint8_t)e8;
      }
    }
  }
}

static int rms_norm_mxfp4_launch(void* aq, int64_t ldaq, uint8_t* a_scale, int64_t ldas, void* out_t, const void* x,
                                 const float* part, int32_t n_splits, const void* weight, void* residual,
                                 int64_t n_tokens, int64_t dim, float eps, int32_t dtype, void* stream) {
  if (n_tokens == 0) return SLM_OK;
  if (n_tokens < 0 || n_tokens >= ((int64_t)1 << 31)) return SLM_ERR_INVALID_ARG;
  if (dim <= 0 || dim % 32 || dim > 16384) return SLM_ERR_UNSUPPORTED;
  if (dtype != SLM_F16 && dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (!aq || !a_scale || (!x && !part) || !weight) return SLM_ERR_INVALID_ARG;
  if (part && n_splits < 1) return SLM_ERR_INVALID_ARG;
  if (ldaq < dim / 2 || ldas < dim / 32) return SLM_ERR_INVALID_ARG;
  if (!aligned16(aq) || ldaq % 16 || (out_t && !aligned16(out_t)) || (x && !aligned16(x)) || (part && !aligned16(part)) ||
      !aligned16(weight) || (residual && !aligned16(residual)))
    return SLM_ERR_ALIGNMENT;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hip_clear_error();
  const int64_t slab = n_tokens * dim;
  const int64_t per_thread = (dim / 8 + 255) / 256;  // slm_rms_norm's NV
  dispatch_dtype(dtype, [&](auto t) {
    using TT = decltype(t);
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)n_tokens), dim3(256), 0, st, reinterpret_cast<char*>(aq), ldaq, a_scale,
                         ldas, reinterpret_cast<uint16_t*>(out_t), reinterpret_cast<const uint16_t*>(x),
                         reinterpret_cast<const uint16_t*>(weight), reinterpret_cast<uint16_t*>(residual), dim, eps, part,
                         (int)n_splits, slab);
    };
    if (per_thread <= 1) go(rms_norm_mxfp4_kernel<TT, 1>);
    else if (per_thread <= 2) go(rms_norm_mxfp4_kernel<TT, 2>);
    else if (per_thread <= 4) go(rms_norm_mxfp4_kernel<TT, 4>);
    else go(rms_norm_mxfp4_kernel<TT, 8>);
  });
  return hip_check_launch();
}

}  // namespace slm

extern "C" {

SLM_API int slm_rms_norm_mxfp4(void* aq, int64_t ldaq, uint8_t* a_scale, int64_t ldas, void* out_t, const void* x,
                               const void* weight, void* residual, int64_t n_tokens, int64_t dim, float eps,
                               int32_t dtype, void* stream) {
  if (n_tokens != 0 && !x) return SLM_ERR_INVALID_ARG;
  return slm::rms_norm_mxfp4_launch(aq, ldaq, a_scale, ldas, out_t, x, nullptr, 0, weight, residual, n_tokens, dim, eps,
                                    dtype, stream);
}

SLM_API int slm_rms_norm_mxfp4_splitk(void* aq, int64_t ldaq, uint8_t* a_scale, int64_t ldas, void* out_t,
                                      const float* partials, int32_t n_splits, const void* weight, void* residual,
                                      int64_t n_tokens, int64_t dim, float eps, int32_t dtype, void* stream) {
  if (n_tokens != 0 && !partials) return SLM_ERR_INVALID_ARG;
  return slm::rms_norm_mxfp4_launch(aq, ldaq, a_scale, ldas, out_t, nullptr, partials, n_splits, weight, residual,
                                    n_tokens, dim, eps, dtype, stream);
}

}  // extern "C"
