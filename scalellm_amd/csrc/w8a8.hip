// w8a8.hip -- fp8 x fp8 linear (W8A8) on the 32x32x64 fp8 MFMA (include/slm_hip.h section 25):
//   slm_w8a8_quantize_act: A[M, K] T -> Aq[M, K] e4m3fn bytes + a_scale[M] fp32 (one scale per token, dynamic, or one
//                          static scale for all of them)
//   slm_w8a8_linear:       C[M, N] = T( ((sum_k e4m3(Aq[m, k]) e4m3(W[n, k])) * a_scale[m]) * w_scale[n] + bias[n] ),
//                          W the checkpoint tensor of section 15
//
// The instruction.  v_mfma_f32_32x32x64_f8f6f4 with both formats e4m3 (cbsz = blgp = 0; the scaled builtin with both
// scale operands the constant 0 assembles to the unscaled form): lane (r = lane & 31, h = lane >> 5) of an operand
// holds 32 bytes of row (column) r in its eight VGPRs -- one half of the step's 64 k -- and the accumulator is the
// 32x32x16 MFMA's: lane (c = lane & 31, h), register 4 j + i = row 8 j + 4 h + i of column c (w4a4.hip's, measured
// there).  NOT MEASURED: which k of the step each of a lane's 32 bytes stands for (the expectation is k = 32 h + byte
// index; no probe with distinct values per byte position was run).  The kernel does not depend on it: it gives lane
// (r, h) of BOTH operands the same 32 consecutive k of the same rows, byte for byte as they lie in memory, so the sum
// runs over matching k whatever order the instruction takes the bytes of a lane in.  What was measured, and is pinned
// by the one-hot sweeps of tests/test_w8a8_exact_gpu.py (hot element on A, then on W, every form, chunk and tail):
// every k of A meets the same k of W and no other, and every (m, n) lands in its place.  Products of e4m3
// values are exact in fp32 and the instruction adds them as an fp32 sum: sums that are exactly representable come out
// exact (the integer tests).
//
// Operands.  Weights are MFMA operand A, activations operand B, as in dense.hip and w4a4.hip: the accumulator tile is
// C^T and the epilogue (slabs, bias, SiLU * mul exchange) is theirs.  K is streamed in dense.hip's 128-deep chunks (the
// plan, the slices and the slabs are section 13's): four 32-byte units per row and chunk, TWO MFMA steps.  Unit order
// (w4a4.hip's block order): step j of a chunk gives lane half h the unit 2 h + j, on both operands -- so a lane's
// weights of a chunk are 64 contiguous bytes of row n: four 16-B global loads, two per step, ZERO converts.  They ride
// in a 3-chunk register ring (16 VGPRs a chunk) that is refilled right after its MFMAs.
//
// Activations are pre-quantised only (a per-token scale needs the whole row before the first byte can be converted)
// and go through LDS, shared by the NW waves of a workgroup on adjacent column tiles: a chunk's image is [rows][8
// slots] x 16 B (slot XOR (row >> 1 & 7): sixteen lanes' ds_read_b128 -- rows r .. r + 15, one slot -- cover all 64
// banks, and so do the sixteen 16-B stores of two rows), double buffered.  Each of the chunk's 8 * rows slots has ONE
// owner thread, 4 RT / NW of them per thread; the A ring (registers, 3 chunks) is stored to the other LDS buffer one
// iteration before its use, dense.hip's pipeline.  Rows beyond M are clamped and never stored.
//
// Tail.  K % 128 leaves 1..3 units: steps of natural order (step s gives lane half h the unit 2 s + h); a lane whose
// unit does not exist feeds zero bytes (e4m3 0x00 = +0) on both operands, so half an MFMA adds exact zeros.
//
// Epilogue.  y = (acc * a_scale[m]) * w_scale[n]: two fp32 multiplies in this order, each kept from contraction
// (fp8_cvt.h: scaled), both scale vectors read once, here.  Slabs are stored scaled.
//
// Forms: RT = 1 / 2 / 4 row tiles per wave, NW = 1 / 2 / 4 >= RT waves, the K split and SiLU * mul exactly as
// dense.hip's (dense_plan.h under the knobs SLM_W8A8_RT / _NW / _SPLITK).  A wave's arithmetic does not depend on the
// form; repeats are bit-identical (no atomics, fixed order).
//
// The quantiser: one workgroup of 256 threads owns one row and holds it in registers (8 values of T per 16-B load, up
// to 16 loads per thread: K <= 32768) between the amax and the convert -- the row is read from HBM once.  amax is
// integer work on the 16-bit patterns (|x| as bits orders like |x|, inf and NaN sort above every finite value);
// s = amax / 448 and x / s are IEEE fp32 divisions, the clamp is at +-448 and the hardware converter
// (v_cvt_scalef32_pk_fp8_f32, scale 1) rounds to nearest even onto e4m3fn keeping the sign of a zero result.
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include <type_traits>

#include "common.h"
#include "dense_plan.h"
#include "fp8_cvt.h"
#include "tuning.h"

namespace slm {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int W8A8_RING = 3;  // weight / A register rings (chunks)

struct W8A8KParams {
  const char* a;         // [M, K] e4m3 bytes
  const float* a_scale;  // [M] or NULL (1.0)
  const char* w;         // [N, K] e4m3 bytes
  const float* w_scale;  // [N] or NULL (1.0)
  const void* bias;      // [N] T or NULL
  void* c;
  float* part;           // [split_k][M][N] or NULL (split_k == 1)
  int64_t lda, ldw;      // bytes
  int64_t ldc;           // elements
  int M, N;
  int n_tiles;     // N / 32
  int tail_units;  // (K % 128) / 32
  int split_k;
  int silu;
  int slice_chunk[LIN_MAX_SPLIT + 1];
};

// D = A . B + C over 64 k: 32 e4m3 bytes per lane and operand
__device__ __forceinline__ f32x16 mfma_f8(const u32x4 a0, const u32x4 a1, const u32x4 b0, const u32x4 b1,
                                          const f32x16 c) {
  const i32x8 av = {(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
  const i32x8 bv = {(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, 0, 0, 0, 0, 0, 0);
}

// byte offset of (row, 16-B slot) in a stage's [rows][128 B] image
__device__ __forceinline__ int a8_off(int row, int slot) { return row * 128 + ((slot ^ ((row >> 1) & 7)) << 4); }

template <typename T, int RT, int NW>
__global__ void __launch_bounds__(NW * 64) w8a8_linear_kernel(const W8A8KParams p) {
  constexpr int RING = W8A8_RING;
  constexpr int NT = NW * 64;
  constexpr int ROWS = RT * 32;
  constexpr int NSLOT = ROWS * 8;   // 16-B slots of a chunk of A
  constexpr int P = NSLOT / NT;     // ... per thread
  constexpr int STAGE = ROWS * 128;
  static_assert(NSLOT % NT == 0 && P >= 1 && P <= 4, "NW >= RT");
  static_assert(NW < 2 || 2 * STAGE >= (NW / 2) * RT * 4 * 64 * 8, "the SiLU exchange fits the stages");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nb = blockIdx.x, ks = blockIdx.y;
  const int row0 = blockIdx.z * ROWS;

  // ---- the wave's column tile (dense.hip) ----
  int nt;
  bool nvalid;
  if (p.silu) {
    const int half_tiles = p.n_tiles >> 1;
    int pi = nb * (NW / 2) + (wave >> 1);
    nvalid = pi < half_tiles;
    if (!nvalid) pi = half_tiles - 1;  // clamped duplicate work, never stored
    nt = (wave & 1) * half_tiles + pi;
  } else {
    nt = nb * NW + wave;
    nvalid = nt < p.n_tiles;
    if (!nvalid) nt = p.n_tiles - 1;
  }
  const int mrow = lane & 31, kh = lane >> 5;

  const int c0 = p.slice_chunk[ks];
  const int nC = p.slice_chunk[ks + 1] - c0;
  const int tail_units = ks == p.split_k - 1 ? p.tail_units : 0;

  // ---- A: this thread's P slots (row, slot) of a chunk; rows beyond M are clamped, never stored ----
  const char* a_src[P];
  int a_dst[P];
  const int a_slot = tid & 7;  // NT % 8 == 0: the same slot in every one of the thread's rows
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int row = (tid + NT * i) >> 3;
    int gr = row0 + row;
    gr = gr < p.M ? gr : p.M - 1;
    a_src[i] = p.a + (int64_t)gr * p.lda + a_slot * 16 + (uint32_t)c0 * 128u;
    a_dst[i] = a8_off(row, a_slot);
  }
  // lane half kh: units 2 kh, 2 kh + 1 of the chunk = 64 contiguous bytes of row n
  const int64_t wrow = (int64_t)nt * 32 + mrow;
  const char* wlane = p.w + wrow * p.ldw + (uint32_t)c0 * 128u;
  const int f_off = mrow * 128;  // + t * 32 * 128: the row's bytes
  const int f_swz = (mrow >> 1) & 7;

  f32x16 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  if (nC > 0) {
    const int last = nC - 1;
    auto clampc = [&](int c) { return c < last ? c : last; };
    u32x4 areg[RING][P];
    u32x4 wreg[RING][4];
    auto a_load = [&](int c, u32x4 (&dst)[P]) {
      const uint32_t cc = (uint32_t)clampc(c);
#pragma unroll
      for (int i = 0; i < P; ++i) dst[i] = *reinterpret_cast<const u32x4*>(a_src[i] + cc * 128u);
    };
    auto a_store = [&](int stage, const u32x4 (&src)[P]) {
#pragma unroll
      for (int i = 0; i < P; ++i) *reinterpret_cast<u32x4*>(smem + stage * STAGE + a_dst[i]) = src[i];
    };
    const char* wl = wlane + kh * 64;
    auto w_load = [&](int c, u32x4 (&w)[4]) {
      const uint32_t cc = (uint32_t)clampc(c);
#pragma unroll
      for (int q = 0; q < 4; ++q) w[q] = *reinterpret_cast<const u32x4*>(wl + cc * 128u + q * 16);
    };

    a_load(0, areg[0]);
    w_load(0, wreg[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int d = 1; d < RING; ++d) {
      a_load(d, areg[d]);
      __builtin_amdgcn_sched_barrier(0);
      w_load(d, wreg[d]);
      __builtin_amdgcn_sched_barrier(0);
    }
    a_store(0, areg[0]);
    __syncthreads();

    int stage = 0;
    const int n_iter = (nC + RING - 1) / RING * RING;
    for (int base = 0; base < n_iter; base += RING) {
#pragma unroll
      for (int u = 0; u < RING; ++u) {
        const int i = base + u;  // chunk; ring slot u
        a_load(i + RING, areg[u]);
        __builtin_amdgcn_sched_barrier(0);
        if (i < nC) {
          const char* sbase = smem + stage * STAGE + f_off;
#pragma unroll
          for (int j = 0; j < 2; ++j) {  // step j: this lane half's unit 2 kh + j = slots 2 unit, 2 unit + 1
            const int slot = 2 * (2 * kh + j);
#pragma unroll
            for (int t = 0; t < RT; ++t) {
              const u32x4 af0 = *reinterpret_cast<const u32x4*>(sbase + t * (32 * 128) + ((slot ^ f_swz) << 4));
              const u32x4 af1 = *reinterpret_cast<const u32x4*>(sbase + t * (32 * 128) + (((slot + 1) ^ f_swz) << 4));
              acc[t] = mfma_f8(wreg[u][2 * j], wreg[u][2 * j + 1], af0, af1, acc[t]);
            }
          }
        }
        // the refill AFTER the old values are consumed (pinned): each ring slot keeps its registers
        __builtin_amdgcn_sched_barrier(0);
        w_load(i + RING, wreg[u]);
        __builtin_amdgcn_sched_barrier(0);
        // chunk i + 1 -> the buffer everybody finished reading one barrier ago
        a_store(stage ^ 1, areg[(u + 1) % RING]);
        __syncthreads();
        stage ^= 1;
      }
    }
  }

  // ---- K % 128 (last slice): up to three units, step s gives lane half kh the unit 2 s + kh ----
  if (tail_units > 0) {
    __syncthreads();  // nobody reads the stages any more
    if ((a_slot >> 1) < tail_units) {
#pragma unroll
      for (int i = 0; i < P; ++i)
        *reinterpret_cast<u32x4*>(smem + a_dst[i]) = *reinterpret_cast<const u32x4*>(a_src[i] + (uint32_t)nC * 128u);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (2 * s < tail_units) {
        const int unit = 2 * s + kh;
        const bool live = unit < tail_units;
        const int uu = live ? unit : 0;  // a lane without a unit: zero bytes, loads stay inside the row
        const char* wsrc = wlane + (uint32_t)nC * 128u + uu * 32;
        u32x4 w0 = *reinterpret_cast<const u32x4*>(wsrc);
        u32x4 w1 = *reinterpret_cast<const u32x4*>(wsrc + 16);
        if (!live) { w0 = u32x4{0, 0, 0, 0}; w1 = w0; }
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          const char* sbase = smem + t * (32 * 128) + f_off;
          u32x4 af0 = *reinterpret_cast<const u32x4*>(sbase + (((2 * uu) ^ f_swz) << 4));
          u32x4 af1 = *reinterpret_cast<const u32x4*>(sbase + (((2 * uu + 1) ^ f_swz) << 4));
          if (!live) { af0 = u32x4{0, 0, 0, 0}; af1 = af0; }
          acc[t] = mfma_f8(w0, w1, af0, af1, acc[t]);
        }
      }
    }
  }
  __syncthreads();  // the SiLU exchange below reuses the stages

  // ---- epilogue (dense.hip's).  C^T layout: lane (m = lane & 31, kh), registers 4 j .. 4 j + 3 = columns
  // 8 j + 4 kh + {0..3}
  const int ncol0 = nt * 32 + 4 * kh;  // + 8 j
  {  // y = (acc * a_scale[m]) * w_scale[n], in place
    float as[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      int gm = row0 + t * 32 + mrow;
      gm = gm < p.M ? gm : p.M - 1;
      as[t] = p.a_scale ? p.a_scale[gm] : 1.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 s = {1.f, 1.f, 1.f, 1.f};
      if (p.w_scale) s = *reinterpret_cast<const f32x4*>(p.w_scale + ncol0 + 8 * j);
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        acc[t][4 * j] = scaled(scaled(acc[t][4 * j], as[t]), s.x);
        acc[t][4 * j + 1] = scaled(scaled(acc[t][4 * j + 1], as[t]), s.y);
        acc[t][4 * j + 2] = scaled(scaled(acc[t][4 * j + 2], as[t]), s.z);
        acc[t][4 * j + 3] = scaled(scaled(acc[t][4 * j + 3], as[t]), s.w);
      }
    }
  }
  if (p.part) {  // a K slice: the fp32 slab, no bias, no rounding
    if (!nvalid) return;
    float* slab = p.part + (int64_t)ks * p.M * p.N;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int gm = row0 + t * 32 + mrow;
      if (gm < p.M) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 v = {acc[t][4 * j], acc[t][4 * j + 1], acc[t][4 * j + 2], acc[t][4 * j + 3]};
          *reinterpret_cast<f32x4*>(slab + (int64_t)gm * p.N + ncol0 + 8 * j) = v;
        }
      }
    }
    return;
  }
  // T( y + bias ), packed pairs
  u32x2 packed[RT][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) {
      const u32x2 bv = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(p.bias) + ncol0 + 8 * j);
      b.x = lo_f32<T>(bv.x); b.y = hi_f32<T>(bv.x); b.z = lo_f32<T>(bv.y); b.w = hi_f32<T>(bv.y);
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      packed[t][j].x = pack2<T>(acc[t][4 * j] + b.x, acc[t][4 * j + 1] + b.y);
      packed[t][j].y = pack2<T>(acc[t][4 * j + 2] + b.z, acc[t][4 * j + 3] + b.w);
    }
  }
  uint16_t* cbase = reinterpret_cast<uint16_t*>(p.c);
  if constexpr (NW >= 2) {
    if (p.silu) {
      // the up wave hands its T-rounded tiles to the gate wave through the (now idle) stages; same lane, same (t, j)
      u32x2* ex = reinterpret_cast<u32x2*>(smem) + (wave >> 1) * (RT * 4 * 64);
      if (wave & 1) {
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int j = 0; j < 4; ++j) ex[(t * 4 + j) * 64 + lane] = packed[t][j];
      }
      __syncthreads();
      if ((wave & 1) || !nvalid) return;
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const int gm = row0 + t * 32 + mrow;
        if (gm < p.M) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const u32x2 g = packed[t][j], u = ex[(t * 4 + j) * 64 + lane];
            u32x2 r;
            r.x = pack2<T>(silu_mul1(lo_f32<T>(g.x), lo_f32<T>(u.x)), silu_mul1(hi_f32<T>(g.x), hi_f32<T>(u.x)));
            r.y = pack2<T>(silu_mul1(lo_f32<T>(g.y), lo_f32<T>(u.y)), silu_mul1(hi_f32<T>(g.y), hi_f32<T>(u.y)));
            *reinterpret_cast<u32x2*>(cbase + (int64_t)gm * p.ldc + ncol0 + 8 * j) = r;  // the gate wave: nt = the output tile
          }
        }
      }
      return;
    }
  }
  if (!nvalid) return;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int gm = row0 + t * 32 + mrow;
    if (gm < p.M) {
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<u32x2*>(cbase + (int64_t)gm * p.ldc + ncol0 + 8 * j) = packed[t][j];
    }
  }
}

// ---- the quantiser: one workgroup per row, the row held in registers between the amax and the convert ----
constexpr int W8A8_QT = 256;         // threads per row
constexpr int W8A8_QMAX_K = 32768;   // 16 loads of 8 values per thread

template <typename T>
struct T16Bits;
template <>
struct T16Bits<bf16_tag> { static constexpr uint32_t INF = 0x7F80u; };
template <>
struct T16Bits<f16_tag> { static constexpr uint32_t INF = 0x7C00u; };

// (the pair convert f32x2_to_e4m3 lives in fp8_cvt.h: the fp8 KV append shares it)
template <typename T, int NV>
__global__ void __launch_bounds__(W8A8_QT) w8a8_quantize_kernel(const char* __restrict__ a, int64_t lda_bytes,
                                                                char* __restrict__ aq, int64_t ldaq,
                                                                float* __restrict__ a_scale,
                                                                const float* __restrict__ static_scale, int nvec) {
  __shared__ uint32_t red[W8A8_QT / 64];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const char* src = a + row * lda_bytes;
  u32x4 x[NV];
  uint32_t mx = 0;  // the largest |x| as a 16-bit pattern
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = tid + W8A8_QT * i;
    if (v < nvec) {
      x[i] = *reinterpret_cast<const u32x4*>(src + (int64_t)v * 16);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const uint32_t lo = x[i][d] & 0x7FFFu, hi = (x[i][d] >> 16) & 0x7FFFu;
        mx = mx > lo ? mx : lo;
        mx = mx > hi ? mx : hi;
      }
    }
  }
  float s;
  if (static_scale) {
    s = *static_scale;
  } else {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)mx, off, 64);
      mx = mx > o ? mx : o;
    }
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < W8A8_QT / 64; ++w) mx = mx > red[w] ? mx : red[w];
    if (mx >= T16Bits<T>::INF) {  // inf or NaN in the row: s = NaN, every code 0x7F
      if (tid == 0) a_scale[row] = __builtin_bit_cast(float, 0x7FC00000u);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int v = tid + W8A8_QT * i;
        if (v < nvec) *reinterpret_cast<u32x2*>(aq + row * ldaq + (int64_t)v * 8) = u32x2{0x7F7F7F7Fu, 0x7F7F7F7Fu};
      }
      return;
    }
    s = mx == 0 ? 1.0f : lo_f32<T>(mx) / 448.0f;
  }
  if (tid == 0) a_scale[row] = s;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = tid + W8A8_QT * i;
    if (v < nvec) {
      float f[8];
      unpack8<T>(x[i], f);
      u32x2 q;
      q.x = f32x2_to_e4m3<false>(0u, f[0] / s, f[1] / s);
      q.x = f32x2_to_e4m3<true>(q.x, f[2] / s, f[3] / s);
      q.y = f32x2_to_e4m3<false>(0u, f[4] / s, f[5] / s);
      q.y = f32x2_to_e4m3<true>(q.y, f[6] / s, f[7] / s);
      *reinterpret_cast<u32x2*>(aq + row * ldaq + (int64_t)v * 8) = q;
    }
  }
}

// ---- host ----
static int plan_w8a8(const slm_w8a8_linear_args* a, LinearPlan* pl) {
  const int rc = plan_linear(a, pl, TUNE_W8A8_RT, TUNE_W8A8_NW, TUNE_W8A8_SPLITK);
  if (rc == SLM_OK) pl->lds_bytes = (uint64_t)2 * pl->rt * 32 * 128;  // two stages of [rows][128 B]
  return rc;
}

template <typename T>
static void launch_w8a8_form(const W8A8KParams& kp, int rt, int nw, dim3 grid, hipStream_t st) {
  if (rt == 4) hipLaunchKernelGGL((w8a8_linear_kernel<T, 4, 4>), grid, dim3(256), 0, st, kp);
  else if (rt == 2 && nw == 4) hipLaunchKernelGGL((w8a8_linear_kernel<T, 2, 4>), grid, dim3(256), 0, st, kp);
  else if (rt == 2) hipLaunchKernelGGL((w8a8_linear_kernel<T, 2, 2>), grid, dim3(128), 0, st, kp);
  else if (nw == 4) hipLaunchKernelGGL((w8a8_linear_kernel<T, 1, 4>), grid, dim3(256), 0, st, kp);
  else if (nw == 2) hipLaunchKernelGGL((w8a8_linear_kernel<T, 1, 2>), grid, dim3(128), 0, st, kp);
  else hipLaunchKernelGGL((w8a8_linear_kernel<T, 1, 1>), grid, dim3(64), 0, st, kp);
}

static int run_w8a8(const slm_w8a8_linear_args* a, void* stream) {
  LinearPlan pl;
  const int rc = plan_w8a8(a, &pl);
  if (rc != SLM_OK) return rc;
  if (a->M == 0) return SLM_OK;
  const bool silu = (a->flags & SLM_LINEAR_SILU_MUL) != 0;
  const bool defer = (a->flags & SLM_LINEAR_DEFER_REDUCE) && !a->bias && pl.split_k > 1;
  if (!a->a || !a->w || !a->c) return SLM_ERR_INVALID_ARG;
  // lda and ldw count bytes
  if (a->lda < a->K || a->ldw < a->K || a->ldc < (silu ? a->N / 2 : a->N)) return SLM_ERR_INVALID_ARG;
  // every row of A, W and C starts on a 16-B boundary; w_scale is read four floats at a time
  if (!aligned16(a->a) || a->lda % 16 || !aligned16(a->w) || a->ldw % 16 || !aligned16(a->c) || a->ldc % 8 ||
      (reinterpret_cast<uintptr_t>(a->bias) & 7u) || !aligned16(a->workspace) || !aligned16(a->w_scale) ||
      (reinterpret_cast<uintptr_t>(a->a_scale) & 3u))
    return SLM_ERR_ALIGNMENT;
  if (pl.ws_bytes > 0 && (!a->workspace || a->workspace_bytes < pl.ws_bytes)) return SLM_ERR_WORKSPACE;

  W8A8KParams kp;
  kp.a = reinterpret_cast<const char*>(a->a);
  kp.a_scale = a->a_scale;
  kp.w = reinterpret_cast<const char*>(a->w);
  kp.w_scale = a->w_scale;
  kp.bias = pl.split_k > 1 ? nullptr : a->bias;  // a split call adds it in the reduce
  kp.c = a->c;
  kp.part = pl.split_k > 1 ? reinterpret_cast<float*>(a->workspace) : nullptr;
  kp.lda = a->lda; kp.ldw = a->ldw; kp.ldc = a->ldc;
  kp.M = (int)a->M; kp.N = (int)a->N;
  kp.n_tiles = (int)(a->N / 32);
  kp.tail_units = pl.tail_units;
  kp.split_k = pl.split_k;
  kp.silu = silu ? 1 : 0;
  for (int j = 0; j <= LIN_MAX_SPLIT; ++j) kp.slice_chunk[j] = pl.slice_chunk[j];
  hip_clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)pl.col_groups, (unsigned)pl.split_k, (unsigned)pl.row_blocks);
  dispatch_dtype(a->dtype, [&](auto t) { launch_w8a8_form<decltype(t)>(kp, pl.rt, pl.nw, grid, st); });
  const int lrc = hip_check_launch();
  if (lrc != SLM_OK || pl.split_k == 1 || defer) return lrc;
  dispatch_dtype(a->dtype, [&](auto t) {
    launch_splitk_reduce<decltype(t)>(kp.part, a->bias, a->c, a->M, a->N, a->ldc, pl.split_k, st);
  });
  return hip_check_launch();
}

template <typename T>
static void launch_w8a8_quantize(const void* a, int64_t lda, void* aq, int64_t ldaq, float* a_scale,
                                 const float* static_scale, int64_t M, int nvec, hipStream_t st) {
  const dim3 grid((unsigned)M), block(W8A8_QT);
  const char* src = reinterpret_cast<const char*>(a);
  char* dst = reinterpret_cast<char*>(aq);
  // the fewest loads per thread that hold the row: K <= 4096, <= 8192, <= 32768
  if (nvec <= 2 * W8A8_QT)
    hipLaunchKernelGGL((w8a8_quantize_kernel<T, 2>), grid, block, 0, st, src, 2 * lda, dst, ldaq, a_scale, static_scale, nvec);
  else if (nvec <= 4 * W8A8_QT)
    hipLaunchKernelGGL((w8a8_quantize_kernel<T, 4>), grid, block, 0, st, src, 2 * lda, dst, ldaq, a_scale, static_scale, nvec);
  else
    hipLaunchKernelGGL((w8a8_quantize_kernel<T, 16>), grid, block, 0, st, src, 2 * lda, dst, ldaq, a_scale, static_scale, nvec);
}

}  // namespace slm

extern "C" {

SLM_API int slm_w8a8_quantize_act(const void* a, int64_t lda, void* aq, int64_t ldaq, float* a_scale,
                                  const float* static_scale, int64_t M, int64_t K, int32_t dtype, void* stream) {
  if (M < 0 || K <= 0) return SLM_ERR_INVALID_ARG;
  if (dtype != SLM_F16 && dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (K % 32 || K > slm::W8A8_QMAX_K || M >= ((int64_t)1 << 30)) return SLM_ERR_UNSUPPORTED;
  if (M == 0) return SLM_OK;
  if (!a || !aq || !a_scale || lda < K || ldaq < K) return SLM_ERR_INVALID_ARG;
  if (!slm::aligned16(a) || lda % 8 || !slm::aligned16(aq) || ldaq % 16 || (reinterpret_cast<uintptr_t>(a_scale) & 3u) ||
      (reinterpret_cast<uintptr_t>(static_scale) & 3u))
    return SLM_ERR_ALIGNMENT;
  slm::hip_clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  slm::dispatch_dtype(dtype, [&](auto t) {
    slm::launch_w8a8_quantize<decltype(t)>(a, lda, aq, ldaq, a_scale, static_scale, M, (int)(K / 8), st);
  });
  return slm::hip_check_launch();
}

SLM_API int slm_w8a8_linear_plan(const slm_w8a8_linear_args* a, slm_linear_plan_info* out) {
  slm::LinearPlan pl;
  if (!out) return SLM_ERR_INVALID_ARG;
  const int rc = slm::plan_w8a8(a, &pl);
  if (rc != SLM_OK) return rc;
  *out = slm_linear_plan_info{};
  out->row_tiles = pl.rt; out->waves = pl.nw;
  out->row_blocks = (int32_t)pl.row_blocks; out->col_groups = (int32_t)pl.col_groups;
  out->split_k = pl.split_k; out->n_chunks = pl.n_chunks; out->tail_units = pl.tail_units;
  for (int j = 0; j <= slm::LIN_MAX_SPLIT; ++j) out->slice_chunk[j] = pl.slice_chunk[j];
  out->lds_bytes = pl.lds_bytes; out->workspace_bytes = pl.ws_bytes;
  return SLM_OK;
}

SLM_API int32_t slm_w8a8_linear_deferred_splits(const slm_w8a8_linear_args* a) {
  slm::LinearPlan pl;
  return slm::plan_w8a8(a, &pl) == SLM_OK && (a->flags & SLM_LINEAR_DEFER_REDUCE) && !a->bias && pl.split_k > 1
             ? pl.split_k : 0;
}

SLM_API int slm_w8a8_linear(const slm_w8a8_linear_args* a, void* stream) { return slm::run_w8a8(a, stream); }

}  // extern "C"
