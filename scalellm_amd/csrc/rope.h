// rope.h -- the rotary-embedding arithmetic every RoPE kernel shares (glue.hip: slm_rope_kv_append and its
// split-K form; mla_glue.hip: slm_mla_rope_append), so that the same values give the same bits in all of them.
#pragma once
#include "common.h"

namespace slm {

// (a, b) rotated by (cos, sin): ONE spelling for every RoPE kernel (explicit fma, so the compiler's
// contraction choices cannot differ between them -- the split-K form must reproduce the plain one)
__device__ __forceinline__ void rope_rot(const float a, const float b, const float c, const float s,
                                         float& o0, float& o1) {
  o0 = __builtin_fmaf(a, c, -(b * s));
  o1 = __builtin_fmaf(b, c, a * s);
  // fp32 results in registers before any conversion to T (otherwise fp16 callers may get a
  // single-rounding v_fma_mixlo_f16 in one kernel and fma + convert in another)
  asm("" : "+v"(o0));
  asm("" : "+v"(o1));
}

// entry i of a cos_sin row held in T (16-bit) or in fp32
template <typename T, typename CS>
__device__ __forceinline__ float rope_cs(const CS* __restrict__ cs, const int i) {
  if constexpr (sizeof(CS) == 4) return (float)cs[i];
  else return lo_f32<T>((uint32_t)cs[i]);
}

// One 4 + 4-value unit u of a head (the thread -> value map of the vector RoPE kernels): a[] holds dims
// [8u, 8u + 4) and b[] dims [8u + 4, 8u + 8) under the interleaved pairing (pairs (2i, 2i + 1)), or a[] dims
// [4u, 4u + 4) and b[] dims [half + 4u, ...) under the other (pairs (i, i + half)).  cs = the position's row
// [cos(half) | sin(half)].
template <typename T, typename CS>
__device__ __forceinline__ void rope_unit8(const float (&a)[4], const float (&b)[4], const CS* __restrict__ cs,
                                           const int half, const int u, const int interleaved, float (&oa)[4],
                                           float (&ob)[4]) {
  if (interleaved) {  // pairs (a0,a1) (a2,a3) (b0,b1) (b2,b3), pair index r = 4u + {0,1,2,3}
    const float c0 = rope_cs<T>(cs, 4 * u), s0 = rope_cs<T>(cs, half + 4 * u);
    const float c1 = rope_cs<T>(cs, 4 * u + 1), s1 = rope_cs<T>(cs, half + 4 * u + 1);
    const float c2 = rope_cs<T>(cs, 4 * u + 2), s2 = rope_cs<T>(cs, half + 4 * u + 2);
    const float c3 = rope_cs<T>(cs, 4 * u + 3), s3 = rope_cs<T>(cs, half + 4 * u + 3);
    rope_rot(a[0], a[1], c0, s0, oa[0], oa[1]);
    rope_rot(a[2], a[3], c1, s1, oa[2], oa[3]);
    rope_rot(b[0], b[1], c2, s2, ob[0], ob[1]);
    rope_rot(b[2], b[3], c3, s3, ob[2], ob[3]);
  } else {            // pairs (a[e], b[e]), r = 4u + e
#pragma unroll
    for (int e = 0; e < 4; ++e)
      rope_rot(a[e], b[e], rope_cs<T>(cs, 4 * u + e), rope_cs<T>(cs, half + 4 * u + e), oa[e], ob[e]);
  }
}

}  // namespace slm
