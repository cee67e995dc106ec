// mxfp4_cvt.h -- the OCP MXFP4 weight side of the weight-stream kernel (dense.hip): e2m1 nibbles with one e8m0 scale
// byte per 32 consecutive k, converted to MFMA weight fragments with the block scale applied IN the converter.
//
// v_cvt_scalef32_pk_{bf16,f16}_fp4 takes a dword, a byte select 0..3 and an fp32 scale and returns a packed pair of
// T: element 0 (the low half of the result) is the byte's LOW nibble, element 1 its high nibble -- the OCP / Quark /
// HF gpt-oss order, in which a byte's low nibble is the lower k.  Confirmed on an MI355X: the code sweep of
// tests/test_mxfp4_exact_gpu.py puts every code through every nibble position and passes with this order (the other
// order would swap every k pair).  The converter reads the scale's exponent field only (e = 0 gives 2^-127, not 0;
// e = 255 gives NaN for every code).  So byte b of a step's dword is the k pair
// (2 b, 2 b + 1) of the step's 8 k, and the four converts of bytes 0..3 ARE the MFMA's weight fragment.
//
// The scale operand is the fp32 number 2^(e - 127) built from the block's e8m0 byte e: bit_cast<float>(e << 23).
// e2m1 values are {0, .5, 1, 1.5, 2, 3, 4, 6}: one mantissa bit, so value * 2^s is exact in T wherever it is a
// normal number of T -- bf16: e in [2, 252], f16: e in [114, 140] (include/slm_hip.h section 20 says what happens
// outside).
#pragma once
#include "common.h"

namespace slm {

// the e8m0 byte of an MX block -> the converter's fp32 scale operand 2^(e - 127)
__device__ __forceinline__ float e8m0_scale(uint32_t e) { return __builtin_bit_cast(float, e << 23); }

// two e2m1 codes (byte B of `w`) times `scale` -> a packed pair of T
template <typename T, int B>
__device__ __forceinline__ uint32_t fp4x2_to_t(uint32_t w, float scale);
template <>
__device__ __forceinline__ uint32_t fp4x2_to_t<bf16_tag, 0>(uint32_t w, float s) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 0));
}
template <>
__device__ __forceinline__ uint32_t fp4x2_to_t<bf16_tag, 1>(uint32_t w, float s) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 1));
}
template <>
__device__ __forceinline__ uint32_t fp4x2_to_t<bf16_tag, 2>(uint32_t w, float s) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 2));
}
template <>
__device__ __forceinline__ uint32_t fp4x2_to_t<bf16_tag, 3>(uint32_t w, float s) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 3));
}
template <>
__device__ __forceinline__ uint32_t fp4x2_to_t<f16_tag, 0>(uint32_t w, float s) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 0));
}
template <>
__device__ __forceinline__ uint32_t fp4x2_to_t<f16_tag, 1>(uint32_t w, float s) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 1));
}
template <>
__device__ __forceinline__ uint32_t fp4x2_to_t<f16_tag, 2>(uint32_t w, float s) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 2));
}
template <>
__device__ __forceinline__ uint32_t fp4x2_to_t<f16_tag, 3>(uint32_t w, float s) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 3));
}

// 8 consecutive k of one MX block (one dword of e2m1 nibbles) -> the MFMA's weight fragment, block scale applied
template <typename T>
__device__ __forceinline__ typename Mfma<T>::frag fp4x8_frag(uint32_t d, float scale) {
  const u32x4 f = {fp4x2_to_t<T, 0>(d, scale), fp4x2_to_t<T, 1>(d, scale), fp4x2_to_t<T, 2>(d, scale),
                   fp4x2_to_t<T, 3>(d, scale)};
  return __builtin_bit_cast(typename Mfma<T>::frag, f);
}

}  // namespace slm
