// fp8_cvt.h -- the fp8 (e4m3fn) weight side of the weight-stream kernels (dense.hip, moe_gemm.hip): the exact
// e4m3 -> T conversion into MFMA weight fragments, the MFMA step's weight fragment of either weight side, and the fp32
// channel-scale multiply.
#pragma once
#include "common.h"

namespace slm {

// the compile-time weight side of a weight-stream kernel (KP::SIDE in dense.hip and moe_gemm.hip)
enum WeightSide { W_T = 0, W_E4M3 = 1, W_MXFP4 = 2 };

// two e4m3 codes (the low or the high half of `w`) -> a packed pair of T, exact
template <typename T, bool HI>
__device__ __forceinline__ uint32_t fp8x2_to_t(uint32_t w);
template <>
__device__ __forceinline__ uint32_t fp8x2_to_t<bf16_tag, false>(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
}
template <>
__device__ __forceinline__ uint32_t fp8x2_to_t<bf16_tag, true>(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true));
}
template <>
__device__ __forceinline__ uint32_t fp8x2_to_t<f16_tag, false>(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false));
}
template <>
__device__ __forceinline__ uint32_t fp8x2_to_t<f16_tag, true>(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true));
}

// 8 consecutive k (two dwords of e4m3) -> the MFMA's weight fragment
template <typename T>
__device__ __forceinline__ typename Mfma<T>::frag fp8x8_frag(uint32_t d0, uint32_t d1) {
  const u32x4 f = {fp8x2_to_t<T, false>(d0), fp8x2_to_t<T, true>(d0), fp8x2_to_t<T, false>(d1),
                   fp8x2_to_t<T, true>(d1)};
  return __builtin_bit_cast(typename Mfma<T>::frag, f);
}

// The weight fragment of one MFMA step out of a 16-B weight load.  T weights: the load is the fragment (8 k).  e4m3
// weights: the load holds 16 k, the fragments of two steps; step h = 0 / 1 of the load takes dwords 0, 1 / 2, 3.
template <typename T, bool FP8>
__device__ __forceinline__ typename Mfma<T>::frag step_frag(const u32x4& w, int h) {
  if constexpr (FP8) return h ? fp8x8_frag<T>(w.z, w.w) : fp8x8_frag<T>(w.x, w.y);
  else return __builtin_bit_cast(typename Mfma<T>::frag, w);
}

// y = acc * s as an fp32 value in a register: the compiler may not contract it into the bias add that follows
__device__ __forceinline__ float scaled(float acc, float s) {
  float y = acc * s;
  asm("" : "+v"(y));
  return y;
}

}  // namespace slm
