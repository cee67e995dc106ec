// w4a4_quant.h -- the MXFP4 activation quantiser's arithmetic (include/slm_hip.h section 22): 32 consecutive k of T
// (one MX block, 64 bytes, four 16-B loads of ONE lane) -> 16 bytes of e2m1 codes + one e8m0 byte.  Shared by the
// stand-alone quantiser, by the GEMM's T side (w4a4.hip), by the quantising SiLU * mul epilogues of the grouped and the
// dense GEMM (w4a4_moe.hip, w4a4.hip: quantize_tile_row) and by the RMSNorm that writes MXFP4 (norm_quant.hip), which
// therefore give the same bits.
//
// The rule is kernels.quantize_mxfp4_weight's:
//   e = clamp(floor(log2 amax) - 2 + 127, 1, 254); an all-zero block 127; a block holding inf or NaN 255
//   code = e2m1( RNE(x * 2^(127 - e)) saturated at 6 ), a byte's low nibble the lower k
//  * amax and e are INTEGER work on the 16-bit patterns (|x| = pattern & 0x7fff orders like the value): packed u16
//    maxima over the block's 16 dwords, then the exponent field.  bf16: field E -> e = max(E - 2, 1) (a subnormal
//    amax, E = 0, is below 2^-126: the low clamp; E <= 254 gives e <= 252: the high clamp is never reached).  f16:
//    field E > 0 -> e = E + 110; a subnormal amax = mant * 2^-24 -> e = msb(mant) + 101; so e is in [101, 140].
//    One lane owns the block: no cross-lane step.
//  * the elements go through v_cvt_scalef32_pk_fp4_{bf16,f16} with the scale operand 2^(e - 127): it DIVIDES by the
//    scale, two elements per instruction, element 0 (the low half of the source dword = the lower k) into the low
//    nibble of the selected byte.  Measured on an MI355X over all 65536 patterns of both types at scales 2^-5, 1 and 4
//    against the rule: round to nearest even onto {0, .5, 1, 1.5, 2, 3, 4, 6}, saturation at 6 (inf included), the sign
//    bit kept (a value that rounds to zero keeps its sign: code 8, which the rule allows) -- no difference, so
//    nothing is redone in VALU.  A NaN element gives code 7; its block's e is 255 anyway.
#pragma once
#include <type_traits>

#include "common.h"

namespace slm {

typedef uint16_t u16x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t,
                            __builtin_elementwise_max(__builtin_bit_cast(u16x2_t, a), __builtin_bit_cast(u16x2_t, b)));
}

// the e8m0 byte of a block whose largest |pattern| is m (15 bits)
template <typename T>
__device__ __forceinline__ uint32_t act_block_e8m0(uint32_t m);
template <>
__device__ __forceinline__ uint32_t act_block_e8m0<bf16_tag>(uint32_t m) {
  const int E = (int)(m >> 7);
  const int e = E - 2 > 1 ? E - 2 : 1;
  return m == 0 ? 127u : E == 255 ? 255u : (uint32_t)e;
}
template <>
__device__ __forceinline__ uint32_t act_block_e8m0<f16_tag>(uint32_t m) {
  const uint32_t E = m >> 10;
  const uint32_t sub = 132u - (uint32_t)__builtin_clz(m | 1u);  // msb(mant) + 101 = (31 - clz) + 101
  return m == 0 ? 127u : E == 31 ? 255u : E > 0 ? E + 110u : sub;
}

// two T (one dword) / scale -> byte B of `old`
template <typename T, int B>
__device__ __forceinline__ uint32_t t2_to_fp4(uint32_t old, uint32_t pair, float scale) {
  if constexpr (std::is_same<T, bf16_tag>::value)
    return __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(old, __builtin_bit_cast(bf16x2_t, pair), scale, B);
  else
    return __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(old, __builtin_bit_cast(f16x2_t, pair), scale, B);
}

// The two halves of the rule, for callers whose block does not sit in one lane's four 16-B loads (the quantising
// epilogue of w4a4_moe.hip holds a row's block in two lanes).
// amax: packed u16 maxima of |pattern| over 8 elements (four dwords) joined to `mx`; act_amax15 folds the two halves
__device__ __forceinline__ uint32_t act_amax_pk(uint32_t mx, const u32x4 x) {
  mx = pk_max_u16(mx, x.x & 0x7fff7fffu);
  mx = pk_max_u16(mx, x.y & 0x7fff7fffu);
  mx = pk_max_u16(mx, x.z & 0x7fff7fffu);
  mx = pk_max_u16(mx, x.w & 0x7fff7fffu);
  return mx;
}
__device__ __forceinline__ uint32_t act_amax15(uint32_t mx) {
  return (mx & 0xffffu) > (mx >> 16) ? (mx & 0xffffu) : (mx >> 16);
}
// 2^(e - 127), the converter's scale operand; e = 255: inf, the codes mean nothing
__device__ __forceinline__ float act_cvt_scale(uint32_t e8) { return __builtin_bit_cast(float, e8 << 23); }
// convert: 8 consecutive k (four dwords of T pairs) / scale -> one dword of codes
template <typename T>
__device__ __forceinline__ uint32_t act_cvt8(const u32x4 x, float scale) {
  uint32_t d = 0;
  d = t2_to_fp4<T, 0>(d, x.x, scale);
  d = t2_to_fp4<T, 1>(d, x.y, scale);
  d = t2_to_fp4<T, 2>(d, x.z, scale);
  d = t2_to_fp4<T, 3>(d, x.w, scale);
  return d;
}

// The quantising SiLU * mul epilogue of the W4A4 GEMMs (w4a4_moe.hip, w4a4.hip): a 32 x 32 output tile in the C^T
// accumulator layout is one MX block per row, held by the two lanes (m, kh = 0 / 1): r[j] = the T pairs of columns
// 8 j + 4 kh + {0..3}.  amax over the lane's 16 columns, then across the halves; then half 0 keeps r[0], r[1] and takes
// the partner's (columns 4 .. 7, 12 .. 15), half 1 keeps r[2], r[3] and takes the partner's (columns 16 .. 19,
// 24 .. 27): 16 consecutive columns from 16 kh, returned as their 8 code bytes (bytes 8 kh .. 8 kh + 7 of the block);
// both lanes get the block's e8m0 byte.  All 64 lanes must call it.
__device__ __forceinline__ uint32_t xor32(uint32_t v) { return (uint32_t)__shfl_xor((int)v, 32); }
template <typename T>
__device__ __forceinline__ u32x2 quantize_tile_row(const u32x2 (&r)[4], const int kh, uint32_t& e8) {
  uint32_t mx = act_amax_pk(0u, u32x4{r[0].x, r[0].y, r[1].x, r[1].y});
  mx = act_amax_pk(mx, u32x4{r[2].x, r[2].y, r[3].x, r[3].y});
  mx = pk_max_u16(mx, xor32(mx));
  e8 = act_block_e8m0<T>(act_amax15(mx));
  const float scale = act_cvt_scale(e8);
  const u32x2 s0 = kh ? r[0] : r[2], s1 = kh ? r[1] : r[3];
  const u32x2 t0 = {xor32(s0.x), xor32(s0.y)}, t1 = {xor32(s1.x), xor32(s1.y)};
  const u32x4 q0 = kh ? u32x4{t0.x, t0.y, r[2].x, r[2].y} : u32x4{r[0].x, r[0].y, t0.x, t0.y};
  const u32x4 q1 = kh ? u32x4{t1.x, t1.y, r[3].x, r[3].y} : u32x4{r[1].x, r[1].y, t1.x, t1.y};
  return u32x2{act_cvt8<T>(q0, scale), act_cvt8<T>(q1, scale)};
}

// one MX block: x[q] holds k = 8 q .. 8 q + 7 of the block.  Returns the 16 code bytes, e8m0 byte in `e8`
template <typename T>
__device__ __forceinline__ u32x4 quantize_act_block(const u32x4 (&x)[4], uint32_t& e8) {
  uint32_t mx = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) mx = act_amax_pk(mx, x[q]);
  e8 = act_block_e8m0<T>(act_amax15(mx));
  const float scale = act_cvt_scale(e8);
  u32x4 r;
#pragma unroll
  for (int q = 0; q < 4; ++q) r[q] = act_cvt8<T>(x[q], scale);
  return r;
}

}  // namespace slm
