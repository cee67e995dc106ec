// w4a4.hip -- MXFP4 x MXFP4 linear on the block-scaled MFMA (include/slm_hip.h section 22):
//   slm_w4a4_quantize_act: A[M, K] T -> Aq[M, K/2] e2m1 codes + Ascale[M, K/32] e8m0 bytes (w4a4_quant.h)
//   slm_w4a4_linear:       C[M, N] = T( sum_k a[m, k] w[n, k] + bias[n] ), a and w the dequantised MXFP4 tensors, W the
//                          checkpoint tensors of section 20, A either pre-quantised or T (quantised as it is loaded)
//
// The instruction.  v_mfma_scale_f32_32x32x64_f8f6f4 with both formats e2m1 (cbsz = blgp = 4): lane (r = lane & 31,
// h = lane >> 5) of an operand holds, in the first four of its eight VGPRs, the 32 codes k = 32 h .. 32 h + 31 of row
// (column) r as they lie in memory -- 16 bytes, a byte's low nibble the lower k -- which is exactly ONE MX block, and
// in byte op_sel (0..3) of its scale VGPR that block's e8m0 byte; the other bytes are ignored.  The accumulator is the
// 32x32x16 MFMA's: lane (c = lane & 31, h), register 4 j + i = row 8 j + 4 h + i of column c.  All of it measured on an
// MI355X (random codes and per-(row, block) scales against float64, garbage in the unselected scale bytes, every
// op_sel) and pinned by tests/test_w4a4_exact_gpu.py.  Products of e2m1 values are exact and the instruction adds them
// to the fp32 accumulator as an fp32 sum: sums that are exactly representable come out exact.
//
// Operands.  Weights are MFMA operand A, activations operand B, as in dense.hip: the accumulator tile is C^T and the
// epilogue (slabs, bias, SiLU * mul) is dense.hip's.  K is streamed in dense.hip's 128-deep chunks (the plan, the
// slices and the slabs are section 13's): four MX blocks per row and chunk, TWO MFMA steps.  Block order: step j of a
// chunk gives lane half h the block 2 h + j, on both operands -- so a lane's weights of a chunk are 32 contiguous bytes
// of row n: two 16-B global loads, each one step's operand with ZERO converts, and its two scale bytes are neighbours
// (blocks 4 c + 2 h + {0, 1} of the scale row; byte loads, the scale row stride carries no alignment, K / 32 may be odd).
// Codes and scale bytes ride together in a 3-chunk register ring that is refilled right after its MFMAs, so the scale
// bytes cost no wait of their own (dense.hip's finding: the two byte loads are kept from merging).
//
// Activations go through LDS, shared by the NW waves of a workgroup on adjacent column tiles: a chunk's image is
// [rows][4 blocks] x 16 B of codes (block slot XOR (row >> 2 & 3): sixteen lanes' ds_read_b128 cover all banks) plus
// [rows][4] scale bytes, double buffered.  Each of the chunk's 4 * rows blocks has ONE owner thread in the workgroup: on
// the T side it loads the block's 64 B (four 16-B loads), quantises it (w4a4_quant.h) and stores 16 B + 1 B; on the
// pre-quantised side it copies 16 B + 1 B.  The quantiser therefore runs once per workgroup, not once per wave, and
// the T side is the quantiser followed by the pre-quantised side bit for bit: the same function of the same 64 bytes,
// and the MFMA sees the same LDS image.  The A ring (registers, 3 chunks) is stored to the other LDS buffer one
// iteration before its use, dense.hip's pipeline.
//
// Tail.  K % 128 leaves 1..3 blocks: steps of natural order (step s gives lane half h the unit 2 s + h); a lane whose
// unit does not exist feeds zero codes (and scale byte 127) on both operands, so half an MFMA adds exact zeros.
//
// Forms: RT = 1 / 2 / 4 row tiles per wave, NW = 1 / 2 / 4 >= RT waves, the K split and SiLU * mul exactly as
// dense.hip's (dense_plan.h under the knobs SLM_W4A4_RT / _NW / _SPLITK).  A wave's arithmetic does not depend on the
// form; repeats are bit-identical (no atomics, fixed order).
//
// slm_w4a4q_linear (section 24): the SiLU * mul form whose gate wave writes its output tile as MXFP4 -- one 32 x 32
// tile is one MX block per row (w4a4_quant.h: quantize_tile_row, shared with w4a4_moe.hip).  A compile-time variant
// (QOUT) of the kernel below: the instantiations of slm_w4a4_linear keep their registers.
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include <type_traits>

#include "common.h"
#include "dense_plan.h"
#include "tuning.h"
#include "w4a4_quant.h"

namespace slm {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int W4A4_RING = 3;  // weight / A register rings (chunks)

struct W4A4KParams {
  const char* a;           // T side: [M, K] T; pre-quantised: [M, K / 2] code bytes
  const uint8_t* a_scale;  // pre-quantised: [M, K / 32] e8m0 bytes
  const char* w;           // [N, K / 2] code bytes
  const uint8_t* w_scale;  // [N, K / 32] e8m0 bytes
  const void* bias;        // [N] T or NULL
  void* c;
  float* part;             // [split_k][M][N] or NULL (split_k == 1)
  int64_t lda;             // bytes
  int64_t ldas, ldw, lds;  // bytes
  int64_t ldc;             // elements
  int M, N;
  int n_tiles;     // N / 32
  int tail_units;  // (K % 128) / 32
  int split_k;
  int silu;
  int slice_chunk[LIN_MAX_SPLIT + 1];
  uint8_t* c_scale;  // QOUT: [M, N / 64] e8m0 bytes; c is then [M, N / 4] code bytes and ldc counts bytes
  int64_t ldcs;
};

// D = A . B + C over 64 k: e2m1 codes of one MX block per lane and operand, their e8m0 bytes in byte 0 of sa / sb
__device__ __forceinline__ f32x16 mfma_mx4(const u32x4 a, const uint32_t sa, const u32x4 b, const uint32_t sb,
                                           const f32x16 c) {
  const i32x8 av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
  const i32x8 bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, 4, 4, 0, (int)sa, 0, (int)sb);
}

// byte offset of (row, block) in a stage's code image
__device__ __forceinline__ int a_code_off(int row, int blk) { return row * 64 + ((blk ^ ((row >> 2) & 3)) << 4); }

// QOUT (slm_w4a4q_linear: always SiLU * mul, split_k = 1, no bias): the gate wave stores its output tile's rows as MX
// blocks, not as T
template <typename T, int RT, int NW, bool AQ, bool QOUT = false>
__global__ void __launch_bounds__(NW * 64) w4a4_linear_kernel(const W4A4KParams p) {
  static_assert(!QOUT || NW >= 2, "the quantising epilogue is the SiLU pair's");
  constexpr int RING = W4A4_RING;
  constexpr int NT = NW * 64;
  constexpr int ROWS = RT * 32;
  constexpr int NBLK = ROWS * 4;                // MX blocks of a chunk of A
  constexpr int P = (NBLK + NT - 1) / NT;       // ... per thread
  constexpr int CODES = ROWS * 64;              // bytes of a stage's code image; the scale bytes follow
  constexpr int STAGE = CODES + ROWS * 4;
  constexpr int AL = AQ ? 1 : 4;                // 16-B loads per block of A
  constexpr int ABYTES = AQ ? 16 : 64;          // bytes of a block in a row of A
  static_assert(P >= 1 && P <= 2 && STAGE % 16 == 0, "NW >= RT");
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

  // ---- A: this thread's P blocks (row, blk) of a chunk; rows beyond M are clamped, never stored ----
  const char* a_src[P];
  const uint8_t* as_src[P];
  int a_dst[P], as_dst[P];
  bool a_own[P];
  int a_blk[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int b = tid + NT * i;
    a_own[i] = b < NBLK;
    const int row = (b >> 2) & (ROWS - 1), blk = b & 3;
    int gr = row0 + row;
    gr = gr < p.M ? gr : p.M - 1;
    a_blk[i] = blk;
    a_src[i] = p.a + (int64_t)gr * p.lda + blk * ABYTES + (uint32_t)c0 * (4u * ABYTES);
    as_src[i] = AQ ? p.a_scale + (int64_t)gr * p.ldas + blk + (uint32_t)c0 * 4u : nullptr;
    a_dst[i] = a_code_off(row, blk);
    as_dst[i] = CODES + row * 4 + blk;
  }
  // lane half kh: blocks 2 kh, 2 kh + 1 of the chunk = 32 contiguous bytes of row n, and their scale bytes
  const int64_t wrow = (int64_t)nt * 32 + mrow;
  const char* wlane = p.w + wrow * p.ldw + (uint32_t)c0 * 64u;
  const uint8_t* slane = p.w_scale + wrow * p.lds + (uint32_t)c0 * 4u;
  uint32_t one = 1;
  asm("" : "+s"(one));  // an opaque offset: the two byte loads are not merged into one 2-byte load (dense.hip)
  const uint8_t* slane1 = slane + one;
  const int f_off = mrow * 64;            // + t * 32 * 64: the row's codes
  const int f_swz = (mrow >> 2) & 3;
  const int fs_off = CODES + mrow * 4;    // + t * 32 * 4: the row's scale bytes

  f32x16 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // a block of A, registers -> the stage: quantised here on the T side
  auto a_store1 = [&](char* stage, int i, const u32x4 (&x)[AL], uint32_t e8) {
    u32x4 codes;
    if constexpr (AQ) codes = x[0];
    else codes = quantize_act_block<T>(x, e8);
    *reinterpret_cast<u32x4*>(stage + a_dst[i]) = codes;
    *reinterpret_cast<uint8_t*>(stage + as_dst[i]) = (uint8_t)e8;
  };

  if (nC > 0) {
    const int last = nC - 1;
    auto clampc = [&](int c) { return c < last ? c : last; };
    u32x4 areg[RING][P][AL];
    uint32_t asreg[RING][P];
    u32x4 wreg[RING][2];
    uint32_t sreg[RING][2];
    auto a_load = [&](int c, u32x4 (&dst)[P][AL], uint32_t (&s)[P]) {
      const uint32_t cc = (uint32_t)clampc(c);
#pragma unroll
      for (int i = 0; i < P; ++i) {
        if (a_own[i]) {
#pragma unroll
          for (int q = 0; q < AL; ++q)
            dst[i][q] = *reinterpret_cast<const u32x4*>(a_src[i] + cc * (4u * ABYTES) + q * 16);
          if constexpr (AQ) s[i] = as_src[i][cc * 4u];
          else s[i] = 0;
        }
      }
    };
    auto a_store = [&](int stage, const u32x4 (&src)[P][AL], const uint32_t (&s)[P]) {
#pragma unroll
      for (int i = 0; i < P; ++i)
        if (a_own[i]) a_store1(smem + stage * STAGE, i, src[i], s[i]);
    };
    const char* wl = wlane + kh * 32;
    auto w_load = [&](int c, u32x4 (&w)[2], uint32_t (&s)[2]) {
      const uint32_t cc = (uint32_t)clampc(c);
      w[0] = *reinterpret_cast<const u32x4*>(wl + cc * 64u);
      w[1] = *reinterpret_cast<const u32x4*>(wl + cc * 64u + 16);
      s[0] = slane[cc * 4u + 2 * kh];
      s[1] = slane1[cc * 4u + 2 * kh];
    };

    a_load(0, areg[0], asreg[0]);
    w_load(0, wreg[0], sreg[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int d = 1; d < RING; ++d) {
      a_load(d, areg[d], asreg[d]);
      __builtin_amdgcn_sched_barrier(0);
      w_load(d, wreg[d], sreg[d]);
      __builtin_amdgcn_sched_barrier(0);
    }
    a_store(0, areg[0], asreg[0]);
    __syncthreads();

    int stage = 0;
    const int n_iter = (nC + RING - 1) / RING * RING;
    for (int base = 0; base < n_iter; base += RING) {
#pragma unroll
      for (int u = 0; u < RING; ++u) {
        const int i = base + u;  // chunk; ring slot u
        a_load(i + RING, areg[u], asreg[u]);
        __builtin_amdgcn_sched_barrier(0);
        if (i < nC) {
          const char* sbase = smem + stage * STAGE;
#pragma unroll
          for (int j = 0; j < 2; ++j) {  // step j: this lane half's block 2 kh + j
            const int blk = 2 * kh + j;
#pragma unroll
            for (int t = 0; t < RT; ++t) {
              const u32x4 af = *reinterpret_cast<const u32x4*>(sbase + t * (32 * 64) + f_off + ((blk ^ f_swz) << 4));
              const uint32_t asc = *reinterpret_cast<const uint8_t*>(sbase + t * (32 * 4) + fs_off + blk);
              acc[t] = mfma_mx4(wreg[u][j], sreg[u][j], af, asc, acc[t]);
            }
          }
        }
        // the refill AFTER the old values are consumed (pinned): each ring slot keeps its registers
        __builtin_amdgcn_sched_barrier(0);
        w_load(i + RING, wreg[u], sreg[u]);
        __builtin_amdgcn_sched_barrier(0);
        // chunk i + 1 -> the buffer everybody finished reading one barrier ago
        a_store(stage ^ 1, areg[(u + 1) % RING], asreg[(u + 1) % RING]);
        __syncthreads();
        stage ^= 1;
      }
    }
  }

  // ---- K % 128 (last slice): up to three blocks, step s gives lane half kh the unit 2 s + kh ----
  if (tail_units > 0) {
    __syncthreads();  // nobody reads the stages any more
#pragma unroll
    for (int i = 0; i < P; ++i) {
      if (a_own[i] && a_blk[i] < tail_units) {
        u32x4 x[AL];
        uint32_t e8 = 0;
#pragma unroll
        for (int q = 0; q < AL; ++q)
          x[q] = *reinterpret_cast<const u32x4*>(a_src[i] + (uint32_t)nC * (4u * ABYTES) + q * 16);
        if constexpr (AQ) e8 = as_src[i][(uint32_t)nC * 4u];
        a_store1(smem, i, x, e8);
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (2 * s < tail_units) {
        const int unit = 2 * s + kh;
        const bool live = unit < tail_units;
        const int uu = live ? unit : 0;  // a lane without a unit: zero codes, loads stay inside the row
        u32x4 wv = *reinterpret_cast<const u32x4*>(wlane + (uint32_t)nC * 64u + uu * 16);
        uint32_t wsc = slane[(uint32_t)nC * 4u + uu];
        if (!live) { wv = u32x4{0, 0, 0, 0}; wsc = 127; }
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          u32x4 af = *reinterpret_cast<const u32x4*>(smem + t * (32 * 64) + f_off + ((uu ^ f_swz) << 4));
          uint32_t asc = *reinterpret_cast<const uint8_t*>(smem + t * (32 * 4) + fs_off + uu);
          if (!live) { af = u32x4{0, 0, 0, 0}; asc = 127; }
          acc[t] = mfma_mx4(wv, wsc, af, asc, acc[t]);
        }
      }
    }
  }
  __syncthreads();  // the SiLU exchange below reuses the stages

  // ---- epilogue (dense.hip's).  C^T layout: lane (m = lane & 31, kh), registers 4 j .. 4 j + 3 = columns
  // 8 j + 4 kh + {0..3}
  const int ncol0 = nt * 32 + 4 * kh;  // + 8 j
  if (!QOUT && p.part) {  // a K slice: the fp32 slab, no bias, no rounding
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
  // T( acc + bias ), packed pairs
  u32x2 packed[RT][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (!QOUT && p.bias) {
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
    if (QOUT || p.silu) {
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
      if constexpr (QOUT) {
        // the tile's row as one MX block (w4a4_quant.h); all 64 lanes take part in the exchanges, rows beyond M
        // (clamped duplicates of row M - 1) are only kept from storing
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          const int gm = row0 + t * 32 + mrow;
          u32x2 r[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const u32x2 g = packed[t][j], u = ex[(t * 4 + j) * 64 + lane];
            r[j].x = pack2<T>(silu_mul1(lo_f32<T>(g.x), lo_f32<T>(u.x)), silu_mul1(hi_f32<T>(g.x), hi_f32<T>(u.x)));
            r[j].y = pack2<T>(silu_mul1(lo_f32<T>(g.y), lo_f32<T>(u.y)), silu_mul1(hi_f32<T>(g.y), hi_f32<T>(u.y)));
          }
          uint32_t e8;
          const u32x2 codes = quantize_tile_row<T>(r, kh, e8);
          if (gm < p.M) {
            *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(p.c) + (int64_t)gm * p.ldc + nt * 16 + kh * 8) = codes;
            if (kh == 0) p.c_scale[(int64_t)gm * p.ldcs + nt] = (uint8_t)e8;
          }
        }
        return;
      }
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

// ---- the stand-alone quantiser: one lane owns one MX block (64 B in, 16 B + 1 B out) ----
template <typename T>
__global__ void __launch_bounds__(256) w4a4_quantize_kernel(const char* __restrict__ a, int64_t lda, char* __restrict__ aq,
                                                            int64_t ldaq, uint8_t* __restrict__ a_scale, int64_t ldas,
                                                            int64_t M, int64_t kblocks) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * kblocks) return;
  const int64_t row = idx / kblocks, blk = idx % kblocks;
  const char* src = a + 2 * (row * lda + blk * 32);
  u32x4 x[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) x[q] = *reinterpret_cast<const u32x4*>(src + q * 16);
  uint32_t e8;
  const u32x4 codes = quantize_act_block<T>(x, e8);
  *reinterpret_cast<u32x4*>(aq + row * ldaq + blk * 16) = codes;
  a_scale[row * ldas + blk] = (uint8_t)e8;
}

// ---- host ----
static int plan_w4a4(const slm_w4a4_linear_args* a, LinearPlan* pl) {
  const int rc = plan_linear(a, pl, TUNE_W4A4_RT, TUNE_W4A4_NW, TUNE_W4A4_SPLITK);
  if (rc == SLM_OK) pl->lds_bytes = (uint64_t)2 * pl->rt * 32 * 68;  // two stages of [rows][64 B codes + 4 scale bytes]
  return rc;
}

template <typename T, int RT, int NW>
static void launch_w4a4(const W4A4KParams& kp, bool aq, dim3 grid, hipStream_t st) {
  if constexpr (NW >= 2) {
    if (kp.c_scale) {
      if (aq) hipLaunchKernelGGL((w4a4_linear_kernel<T, RT, NW, true, true>), grid, dim3(NW * 64), 0, st, kp);
      else hipLaunchKernelGGL((w4a4_linear_kernel<T, RT, NW, false, true>), grid, dim3(NW * 64), 0, st, kp);
      return;
    }
  }
  if (aq) hipLaunchKernelGGL((w4a4_linear_kernel<T, RT, NW, true>), grid, dim3(NW * 64), 0, st, kp);
  else hipLaunchKernelGGL((w4a4_linear_kernel<T, RT, NW, false>), grid, dim3(NW * 64), 0, st, kp);
}

template <typename T>
static void launch_w4a4_form(const W4A4KParams& kp, bool aq, int rt, int nw, dim3 grid, hipStream_t st) {
  if (rt == 4) launch_w4a4<T, 4, 4>(kp, aq, grid, st);
  else if (rt == 2 && nw == 4) launch_w4a4<T, 2, 4>(kp, aq, grid, st);
  else if (rt == 2) launch_w4a4<T, 2, 2>(kp, aq, grid, st);
  else if (nw == 4) launch_w4a4<T, 1, 4>(kp, aq, grid, st);
  else if (nw == 2) launch_w4a4<T, 1, 2>(kp, aq, grid, st);
  else launch_w4a4<T, 1, 1>(kp, aq, grid, st);
}

// the flags slm_w4a4q_linear takes: SiLU * mul, no bias, no deferred reduce
static int check_w4a4q(const slm_w4a4_linear_args* a) {
  if (!a) return SLM_ERR_INVALID_ARG;
  if (!(a->flags & SLM_LINEAR_SILU_MUL) || (a->flags & SLM_LINEAR_DEFER_REDUCE) || a->bias) return SLM_ERR_INVALID_ARG;
  return SLM_OK;
}

// c_scale != NULL: slm_w4a4q_linear (c: code bytes, ldc in bytes)
static int run_w4a4(const slm_w4a4_linear_args* a, uint8_t* c_scale, int64_t ldcs, bool qout, void* stream) {
  LinearPlan pl;
  int rc = qout ? check_w4a4q(a) : SLM_OK;
  if (rc == SLM_OK) rc = plan_w4a4(a, &pl);
  if (rc != SLM_OK) return rc;
  if (a->M == 0) return SLM_OK;
  if (qout && !c_scale) return SLM_ERR_INVALID_ARG;
  const bool aq = a->a_scale != nullptr;
  const bool silu = (a->flags & SLM_LINEAR_SILU_MUL) != 0;
  const bool defer = (a->flags & SLM_LINEAR_DEFER_REDUCE) && !a->bias && pl.split_k > 1;
  if (!a->a || !a->w || !a->c || !a->w_scale) return SLM_ERR_INVALID_ARG;
  // lda counts T on the T side and bytes (two codes) on the pre-quantised side; ldw bytes
  if (a->lda < (aq ? a->K / 2 : a->K) || a->ldw < a->K / 2 || a->lds < a->K / 32 || (aq && a->ldas < a->K / 32) ||
      a->ldc < (qout ? a->N / 4 : silu ? a->N / 2 : a->N) || (qout && ldcs < a->N / 64))
    return SLM_ERR_INVALID_ARG;
  // every row of A, W and C starts on a 16-B boundary
  if (!aligned16(a->a) || a->lda % (aq ? 16 : 8) || !aligned16(a->w) || a->ldw % 16 || !aligned16(a->c) || a->ldc % (qout ? 16 : 8) ||
      (reinterpret_cast<uintptr_t>(a->bias) & 7u) || !aligned16(a->workspace))
    return SLM_ERR_ALIGNMENT;
  if (pl.ws_bytes > 0 && (!a->workspace || a->workspace_bytes < pl.ws_bytes)) return SLM_ERR_WORKSPACE;

  W4A4KParams kp;
  kp.a = reinterpret_cast<const char*>(a->a);
  kp.a_scale = a->a_scale;
  kp.w = reinterpret_cast<const char*>(a->w);
  kp.w_scale = a->w_scale;
  kp.bias = pl.split_k > 1 ? nullptr : a->bias;  // a split call adds it in the reduce
  kp.c = a->c;
  kp.part = pl.split_k > 1 ? reinterpret_cast<float*>(a->workspace) : nullptr;
  kp.lda = aq ? a->lda : 2 * a->lda;
  kp.ldas = a->ldas; kp.ldw = a->ldw; kp.lds = a->lds; kp.ldc = a->ldc;
  kp.M = (int)a->M; kp.N = (int)a->N;
  kp.n_tiles = (int)(a->N / 32);
  kp.tail_units = pl.tail_units;
  kp.split_k = pl.split_k;
  kp.silu = silu ? 1 : 0;
  kp.c_scale = qout ? c_scale : nullptr;
  kp.ldcs = ldcs;
  for (int j = 0; j <= LIN_MAX_SPLIT; ++j) kp.slice_chunk[j] = pl.slice_chunk[j];
  hip_clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)pl.col_groups, (unsigned)pl.split_k, (unsigned)pl.row_blocks);
  dispatch_dtype(a->dtype, [&](auto t) { launch_w4a4_form<decltype(t)>(kp, aq, pl.rt, pl.nw, grid, st); });
  const int lrc = hip_check_launch();
  if (lrc != SLM_OK || pl.split_k == 1 || defer) return lrc;
  dispatch_dtype(a->dtype, [&](auto t) {
    launch_splitk_reduce<decltype(t)>(kp.part, a->bias, a->c, a->M, a->N, a->ldc, pl.split_k, st);
  });
  return hip_check_launch();
}

}  // namespace slm

extern "C" {

SLM_API int slm_w4a4_quantize_act(const void* a, int64_t lda, void* aq, int64_t ldaq, uint8_t* a_scale, int64_t ldas,
                                  int64_t M, int64_t K, int32_t dtype, void* stream) {
  if (M < 0 || K <= 0) return SLM_ERR_INVALID_ARG;
  if (dtype != SLM_F16 && dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (K % 32 || K >= ((int64_t)1 << 30) || M >= ((int64_t)1 << 30)) return SLM_ERR_UNSUPPORTED;
  if (M == 0) return SLM_OK;
  if (!a || !aq || !a_scale || lda < K || ldaq < K / 2 || ldas < K / 32) return SLM_ERR_INVALID_ARG;
  if (!slm::aligned16(a) || lda % 8 || !slm::aligned16(aq) || ldaq % 16) return SLM_ERR_ALIGNMENT;
  const int64_t kblocks = K / 32, n = M * kblocks;
  slm::hip_clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  slm::dispatch_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(slm::w4a4_quantize_kernel<decltype(t)>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const char*>(a), lda, reinterpret_cast<char*>(aq), ldaq, a_scale, ldas, M,
                       kblocks);
  });
  return slm::hip_check_launch();
}

SLM_API int slm_w4a4_linear_plan(const slm_w4a4_linear_args* a, slm_linear_plan_info* out) {
  slm::LinearPlan pl;
  if (!out) return SLM_ERR_INVALID_ARG;
  const int rc = slm::plan_w4a4(a, &pl);
  if (rc != SLM_OK) return rc;
  *out = slm_linear_plan_info{};
  out->row_tiles = pl.rt; out->waves = pl.nw;
  out->row_blocks = (int32_t)pl.row_blocks; out->col_groups = (int32_t)pl.col_groups;
  out->split_k = pl.split_k; out->n_chunks = pl.n_chunks; out->tail_units = pl.tail_units;
  for (int j = 0; j <= slm::LIN_MAX_SPLIT; ++j) out->slice_chunk[j] = pl.slice_chunk[j];
  out->lds_bytes = pl.lds_bytes; out->workspace_bytes = pl.ws_bytes;
  return SLM_OK;
}

SLM_API int32_t slm_w4a4_linear_deferred_splits(const slm_w4a4_linear_args* a) {
  slm::LinearPlan pl;
  return slm::plan_w4a4(a, &pl) == SLM_OK && (a->flags & SLM_LINEAR_DEFER_REDUCE) && !a->bias && pl.split_k > 1
             ? pl.split_k : 0;
}

SLM_API int slm_w4a4_linear(const slm_w4a4_linear_args* a, void* stream) {
  return slm::run_w4a4(a, nullptr, 0, false, stream);
}

SLM_API int slm_w4a4q_linear_plan(const slm_w4a4_linear_args* a, slm_linear_plan_info* out) {
  const int rc = slm::check_w4a4q(a);
  return rc == SLM_OK ? slm_w4a4_linear_plan(a, out) : rc;
}

SLM_API int slm_w4a4q_linear(const slm_w4a4_linear_args* a, uint8_t* c_scale, int64_t ldcs, void* stream) {
  return slm::run_w4a4(a, c_scale, ldcs, true, stream);
}

}  // extern "C"
