// common.h -- shared device helpers for libslm_hip (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slm_hip.h"

namespace slm {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

struct bf16_tag {};
struct f16_tag {};

// ---- packed 16-bit pair <-> fp32 ------------------------------------------------
template <typename T>
__device__ __forceinline__ float lo_f32(uint32_t w);
template <typename T>
__device__ __forceinline__ float hi_f32(uint32_t w);

template <>
__device__ __forceinline__ float lo_f32<bf16_tag>(uint32_t w) {
  return __builtin_bit_cast(float, w << 16);
}
template <>
__device__ __forceinline__ float hi_f32<bf16_tag>(uint32_t w) {
  return __builtin_bit_cast(float, w & 0xffff0000u);
}
template <>
__device__ __forceinline__ float lo_f32<f16_tag>(uint32_t w) {
  return (float)__builtin_bit_cast(f16x2_t, w)[0];
}
template <>
__device__ __forceinline__ float hi_f32<f16_tag>(uint32_t w) {
  return (float)__builtin_bit_cast(f16x2_t, w)[1];
}

// fp32 pair -> packed 16-bit pair, round-to-nearest-even
template <typename T>
__device__ __forceinline__ uint32_t pack2(float a, float b);
template <>
__device__ __forceinline__ uint32_t pack2<bf16_tag>(float a, float b) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
template <>
__device__ __forceinline__ uint32_t pack2<f16_tag>(float a, float b) {
  f16x2_t h = {(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(uint32_t, h);
}

template <typename T>
__device__ __forceinline__ uint16_t pack1(float a) {
  return (uint16_t)(pack2<T>(a, 0.f) & 0xffffu);
}

// acc += a.lo*b.lo + a.hi*b.hi  (v_dot2c_f32_bf16 / v_dot2c_f32_f16, fp32 accumulate)
template <typename T>
__device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float acc);
template <>
__device__ __forceinline__ float dot2<bf16_tag>(uint32_t a, uint32_t b, float acc) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a),
                                         __builtin_bit_cast(bf16x2_t, b), acc, false);
}
template <>
__device__ __forceinline__ float dot2<f16_tag>(uint32_t a, uint32_t b, float acc) {
  return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, a), __builtin_bit_cast(f16x2_t, b),
                                acc, false);
}

// D = A . B + C on the matrix pipe: v_mfma_f32_32x32x16_{bf16,f16}, 8 k-values per lane and operand
template <typename T>
struct Mfma;
template <>
struct Mfma<bf16_tag> {
  typedef bf16x8_t frag;
  static __device__ __forceinline__ f32x16 run(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Mfma<f16_tag> {
  typedef f16x8_t frag;
  static __device__ __forceinline__ f32x16 run(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

// ---- cross-lane (wave64) --------------------------------------------------------
// DPP lane exchange inside a row of 16 lanes; full-rate VALU, no LDS traffic.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
constexpr int DPP_QUAD_XOR1 = 0xB1;     // quad_perm:[1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;     // quad_perm:[2,3,0,1]
constexpr int DPP_ROW_HALF_MIRROR = 0x141;  // i <-> 7-i inside each 8 lanes
constexpr int DPP_ROW_MIRROR = 0x140;       // i <-> 15-i inside each 16 lanes

// all-reduce sum across aligned groups of W lanes (W = 4, 8, 16, 32)
template <int W>
__device__ __forceinline__ float group_sum(float v) {
  v += dpp_f32<DPP_QUAD_XOR1>(v);
  v += dpp_f32<DPP_QUAD_XOR2>(v);
  if constexpr (W >= 8) v += dpp_f32<DPP_ROW_HALF_MIRROR>(v);
  if constexpr (W >= 16) v += dpp_f32<DPP_ROW_MIRROR>(v);
  if constexpr (W >= 32) v += __shfl_xor(v, 16, 64);
  if constexpr (W >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}

// all-reduce N independent values across aligned groups of W lanes, one DPP step at a time over
// all N values (keeps N independent dependency chains adjacent in program order)
template <int W, int N>
__device__ __forceinline__ void group_sum_many(float* v) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_f32<DPP_QUAD_XOR1>(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_f32<DPP_QUAD_XOR2>(v[i]);
  if constexpr (W >= 8) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_f32<DPP_ROW_HALF_MIRROR>(v[i]);
  }
  if constexpr (W >= 16) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_f32<DPP_ROW_MIRROR>(v[i]);
  }
  if constexpr (W >= 32) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], 16, 64);
  }
}

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// silu(gate) * up in fp32 on values that are already exact in T: THE formula of the SiLU*mul glue
// kernel (kernel::act_and_mul, reference src/kernels/activation_kernels.cu:84), shared with the
// GEMM epilogues that fuse it so that both paths give identical bits
//
// sigmoid(g) = 1 / (1 + 2^(-g log2 e)) is an fp32 subnormal below g = -87.3, and v_rcp_f32 flushes a
// subnormal result to zero (below -88.7 the exp2 overflows as well), while g * sigmoid(g) * u is still
// a NORMAL bf16 number there: silu(-88) = -5.3e-37 came out as 0.  So below g = -64 the sigmoid is
// carried times 2^32 (exponent argument - 32, 2^-32 in place of the 1) and the product is scaled back
// at the end by an ordinary multiply, which keeps subnormals.  Everywhere else k = 0 and one = 1: the
// fma rounds -g log2 e exactly as the multiply did and x * 1 is x, so those bits are what they were.
// The fma is explicit so that no caller's contraction choice can differ from another's.
__device__ __forceinline__ float silu_mul1(const float g, const float u) {
  const bool tiny = g < -64.0f;
  const float k = tiny ? 32.0f : 0.0f, one = tiny ? 0x1p-32f : 1.0f;
  const float sig = __builtin_amdgcn_rcpf(one + fast_exp2(__builtin_fmaf(-g, 1.4426950408889634f, -k)));
  float r = g * sig * u * one;
  // the product is an fp32 value in a register before any conversion to T: without this the
  // compiler may fold "multiply, then round to fp16" into one v_fma_mixlo_f16 (single rounding) in
  // some callers and not in others (v_pk_mul_f32 + v_cvt), and the fused / unfused paths would
  // differ in the last bit on ties
  asm("" : "+v"(r));
  return r;
}

// the fused-epilogue form: fp32 accumulators -> rounded to T (what the unfused GEMM would have
// stored) -> silu_mul1
template <typename T>
__device__ __forceinline__ float silu_mul_acc(const float gate_acc, const float up_acc) {
  return silu_mul1(lo_f32<T>((uint32_t)pack1<T>(gate_acc)), lo_f32<T>((uint32_t)pack1<T>(up_acc)));
}

// 8 x silu_mul1, rounded RN to T
template <typename T>
__device__ __forceinline__ u32x4 silu_mul8(const u32x4 g, const u32x4 u) {
  const float gf[8] = {lo_f32<T>(g.x), hi_f32<T>(g.x), lo_f32<T>(g.y), hi_f32<T>(g.y),
                       lo_f32<T>(g.z), hi_f32<T>(g.z), lo_f32<T>(g.w), hi_f32<T>(g.w)};
  const float uf[8] = {lo_f32<T>(u.x), hi_f32<T>(u.x), lo_f32<T>(u.y), hi_f32<T>(u.y),
                       lo_f32<T>(u.z), hi_f32<T>(u.z), lo_f32<T>(u.w), hi_f32<T>(u.w)};
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = silu_mul1(gf[j], uf[j]);
  u32x4 r;
  r.x = pack2<T>(o[0], o[1]); r.y = pack2<T>(o[2], o[3]);
  r.z = pack2<T>(o[4], o[5]); r.w = pack2<T>(o[6], o[7]);
  return r;
}

// sum over split-K partial slabs of 4 consecutive columns, in THE order of the split-K reduce
// kernel (below) -- shared with the RMSNorm that can absorb the reduction (glue.hip), so that
// "GEMM -> reduce -> norm" and "GEMM (deferred) -> norm" give identical bits
__device__ __forceinline__ f32x4 splitk_sum4(const float* __restrict__ src, const int64_t slab,
                                             const int split_k) {
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  int k = 0;
  for (; k + 8 <= split_k; k += 8) {  // 8 independent 16-B loads in flight per thread
    f32x4 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const f32x4*>(src + (k + i) * slab);
#pragma unroll
    for (int i = 0; i < 8; ++i) s += v[i];
  }
  for (; k + 2 <= split_k; k += 2) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + k * slab);
    const f32x4 b = *reinterpret_cast<const f32x4*>(src + (k + 1) * slab);
    s += a + b;
  }
  if (k < split_k) s += *reinterpret_cast<const f32x4*>(src + k * slab);
  return s;
}

// 8 packed values of T -> fp32
template <typename T>
__device__ __forceinline__ void unpack8(const u32x4 a, float (&f)[8]) {
  f[0] = lo_f32<T>(a.x); f[1] = hi_f32<T>(a.x); f[2] = lo_f32<T>(a.y); f[3] = hi_f32<T>(a.y);
  f[4] = lo_f32<T>(a.z); f[5] = hi_f32<T>(a.z); f[6] = lo_f32<T>(a.w); f[7] = hi_f32<T>(a.w);
}

// T(sum over slabs) of 8 consecutive columns: the bits the split-K reduce kernel would have stored (the deferred
// consumers mla_glue.hip and qk_norm.hip)
template <typename T>
__device__ __forceinline__ u32x4 slab_sum8(const float* __restrict__ src, const int64_t slab, const int n_splits) {
  const f32x4 s0 = splitk_sum4(src, slab, n_splits);
  const f32x4 s1 = splitk_sum4(src + 4, slab, n_splits);
  u32x4 a;
  a.x = pack2<T>(s0.x, s0.y); a.y = pack2<T>(s0.z, s0.w);
  a.z = pack2<T>(s1.x, s1.y); a.w = pack2<T>(s1.z, s1.w);
  return a;
}

// C[m, n] = T( sum_s part[s][m][n] + bias[n] ): THE split-K reduce (w4.hip, dense.hip).  A deferred consumer
// (splitk_sum4, the same order) and this launch give identical bits
template <typename T>
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const float* __restrict__ part,
                                                            const void* __restrict__ bias,
                                                            void* __restrict__ c, int64_t M,
                                                            int64_t N, int64_t ldc, int split_k) {
  const int64_t idx4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // 4 columns per thread
  if (idx4 * 4 >= M * N) return;
  const int64_t m = (idx4 * 4) / N, n = (idx4 * 4) % N;
  f32x4 s = splitk_sum4(part + m * N + n, M * N, split_k);
  if (bias) {
    const u32x2 b = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(bias) + n);
    s.x += lo_f32<T>(b.x); s.y += hi_f32<T>(b.x);
    s.z += lo_f32<T>(b.y); s.w += hi_f32<T>(b.y);
  }
  u32x2 r;
  r.x = pack2<T>(s.x, s.y);
  r.y = pack2<T>(s.z, s.w);
  *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(c) + m * ldc + n) = r;
}
template <typename T>
inline void launch_splitk_reduce(const float* part, const void* bias, void* c, int64_t M, int64_t N, int64_t ldc,
                                 int split_k, hipStream_t st) {
  const int64_t n4 = M * N / 4;
  hipLaunchKernelGGL(splitk_reduce_kernel<T>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, part, bias, c, M,
                     N, ldc, split_k);
}

// byte offset of (row, 16-B slot) in a [rows][128 k] stage buffer of the weight-stream loops (w4_stream32.h,
// dense.hip, moe_gemm.hip); the XOR swizzle makes the MFMA fragments conflict-free ds_read_b128
__device__ __forceinline__ int stage_swz(int row, int slot) { return row * 256 + ((slot ^ (row & 15)) << 4); }

// ---- what the unquantised GEMMs' hosts share (dense.hip, moe_gemm.hip) ----
constexpr int MI355X_CUS = 256;
// Workgroups per row block: NW adjacent 32-column tiles each, or NW / 2 (gate, up) pairs under SiLU * mul
inline int64_t gemm_col_groups(int64_t n_tiles, int nw, bool silu) {
  return silu ? (n_tiles / 2 + nw / 2 - 1) / (nw / 2) : (n_tiles + nw - 1) / nw;
}

// RMSNorm row arithmetic shared by rms_norm_kernel (glue.hip) and the fused all-reduce
// (allreduce.hip) -- normalization.h:17-52.  The fma is EXPLICIT: left to -ffp-contract the compiler
// fuses or not per kernel, and the two paths would differ in the last bit of the sum of squares.
__device__ __forceinline__ float rms_sumsq8(const float (&f)[8], float ss) {
#pragma unroll
  for (int j = 0; j < 8; ++j) ss = __builtin_fmaf(f[j], f[j], ss);
  return ss;
}
// the row's scale from its sum of squares: shared by rms_norm_kernel and the MLA prologue (mla_glue.hip)
__device__ __forceinline__ float rms_rstd(const float sumsq, const float dim, const float eps) {
  return rsqrtf(sumsq / dim + eps);
}
// y = T(T(h * rs) * w): the normalised value is rounded to T before the weight (normalization.h:27-29)
template <typename T>
__device__ __forceinline__ u32x4 rms_apply8(const float (&h)[8], const float rs, const u32x4 wv) {
  const float wf[8] = {lo_f32<T>(wv.x), hi_f32<T>(wv.x), lo_f32<T>(wv.y), hi_f32<T>(wv.y),
                       lo_f32<T>(wv.z), hi_f32<T>(wv.z), lo_f32<T>(wv.w), hi_f32<T>(wv.w)};
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float n16 = lo_f32<T>((uint32_t)pack1<T>(h[j] * rs));
    o[j] = n16 * wf[j];
  }
  u32x4 r;
  r.x = pack2<T>(o[0], o[1]); r.y = pack2<T>(o[2], o[3]);
  r.z = pack2<T>(o[4], o[5]); r.w = pack2<T>(o[6], o[7]);
  return r;
}

// hipGetLastError() is per-thread sticky state shared with every other HIP user in the process
// (torch, RCCL): clear stale errors when an entry point starts, so that hip_check_launch()
// reports only OUR launch.
inline int& hip_last_error_slot() {
  static thread_local int e = 0;
  return e;
}
inline void hip_clear_error() { (void)hipGetLastError(); }
inline int hip_check_launch() {
  const hipError_t e = hipGetLastError();
  hip_last_error_slot() = (int)e;
  return e == hipSuccess ? SLM_OK : SLM_ERR_LAUNCH;
}

// f(bf16_tag{}) or f(f16_tag{}) for a dtype the caller has checked to be one of the two
template <typename F>
inline void dispatch_dtype(int dtype, F&& f) {
  if (dtype == SLM_BF16) f(bf16_tag{});
  else f(f16_tag{});
}

inline bool is_pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }
inline int ilog2(int64_t x) {
  int r = 0;
  while ((1ll << (r + 1)) <= x) ++r;
  return r;
}
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace slm
