// fp8_cvt.h -- what the fp8 (e4m3fn) weight-only kernels share (dense_fp8.hip, moe_gemm_fp8.hip): the exact
// e4m3 -> T conversion into MFMA weight fragments, and the fp32 channel-scale multiply.
#pragma once
#include "common.h"

namespace slm {

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

// y = acc * s as an fp32 value in a register: the compiler may not contract it into the bias add that follows
__device__ __forceinline__ float scaled(float acc, float s) {
  float y = acc * s;
  asm("" : "+v"(y));
  return y;
}

}  // namespace slm
