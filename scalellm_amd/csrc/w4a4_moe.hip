// w4a4_moe.hip -- grouped MXFP4 x MXFP4 GEMM over the experts of a mixture-of-experts layer on the block-scaled MFMA
// (include/slm_hip.h section 23, slm_moe_w4a4_gemm): moe_gemm.hip's aligned-list contract with w4a4.hip's arithmetic.
//
// For every 32-row block b of the aligned token list (slm_moe_align_block with block_size 32), e = expert_ids[b],
// idx = sorted[b * 32 + r]:
//     C[idx, n] = T( (sum_k a[idx / a_div, k] * w_e[n, k]) * row_scale[idx] ),   one rounding
// a and w_e the dequantised values of two MXFP4 tensors: the experts are section 21's checkpoint tensors ([E, N, K/2]
// code bytes, [E, N, K/32] e8m0 bytes), the activations are PRE-QUANTISED (slm_w4a4_quantize_act, once per token: the
// rule is per row and per 32 k, so it commutes with the gather idx / a_div).  There is no T side: in a grouped GEMM
// every column group of a row block would quantise the same 32 rows again.
//
// One wave, one tile.  A wave owns one 32 x 32 output tile over the whole K; a workgroup is NW = 4 / 2 / 1 waves on
// adjacent column tiles (SiLU * mul: (gate, up) pairs) sharing the LDS image of the block's 32 gathered rows; the host
// takes moe_gemm_waves(max_blocks, n_tiles, silu).  The wave's MFMA sequence over k is w4a4_linear_kernel's at RT = 1
// and split_k = 1, statement for statement: weights are MFMA operand A, activations operand B (the accumulator is the
// C^T tile: lane (m = lane & 31, h = lane >> 5) holds row m, registers 4 j .. 4 j + 3 = columns 8 j + 4 h + {0..3});
// K in 128-deep chunks, TWO v_mfma_scale_f32_32x32x64_f8f6f4 per chunk, step j giving lane half h the block 2 h + j on
// both operands; codes and scale bytes in a 3-chunk register ring refilled right after its MFMAs, the two scale-byte
// loads of a chunk kept from merging; K % 128 in steps of natural order (step s: unit 2 s + h), a lane without a unit
// feeding zero codes and scale byte 127.  So no result bit depends on NW, and an expert's rows are slm_w4a4_linear
// (pre-quantised side, SLM_W4A4_SPLITK = 1) on those rows bit for bit.  The loop is written out here and not shared
// with w4a4.hip through a header: moved into a forceinline function it cost w4a4.hip's RT = 4 forms 60 VGPRs (240 ->
// 304), so w4a4.hip stays as it is; what the two DO share is the quantiser's arithmetic (w4a4_quant.h).
//
// A through LDS.  A chunk's image is w4a4.hip's at one row tile: [32 rows][4 blocks] x 16 B of codes (block slot XOR
// (row >> 2 & 3)) + [32][4] scale bytes = 2176 B, double buffered.  Each of the chunk's 128 blocks has ONE owner thread
// in the workgroup (NW = 1: two per thread; NW = 4: the first 128 threads), which copies 16 B + 1 B of the gathered row;
// the owner's ring is stored to the other buffer one iteration before its use.  One barrier per chunk (two MFMAs);
// staging two chunks per barrier was not measured, so there is no such variant.
//
// Addresses.  Dead blocks (beyond n_padded) and expert ids outside [0, E) leave before any address is formed.  Row n =
// nt * 32 + (lane & 31) < N because nt is clamped to a valid tile.  A ring load of chunk c reads bytes
// [64 cc + 32 h, + 32) of the row with cc = min(c, n_chunks - 1): below 64 n_chunks <= K / 2; a tail load reads
// [64 n_chunks + 16 u, + 16) with u < tail_units: below K / 2.  The scale index is clamped by the same cc:
// 4 cc + 2 h + {0, 1} <= 4 n_chunks - 1, and the tail's 4 n_chunks + u < K / 32.  The host checks ldw >= K / 2, lds >=
// K / 32 and both expert strides >= (N - 1) * stride + row length: no byte outside expert e's own [N, K / 2] and
// [N, K / 32] rows is read, whatever the padding holds.  A: a padding id (>= n_flat) is clamped to row 0, a live one
// reads row idx / a_div, bytes [64 cc + 16 blk, + 16) and scale byte 4 cc + blk under the same clamp.
//
// Epilogues.  Plain / row_scale: fp32 multiply, one rounding, 8-byte stores (C 8-byte aligned, ldc % 4 == 0).
// SLM_MOE_SILU_MUL: w4a4.hip's -- the up wave hands its T-rounded tile to the gate wave through the idle stages: the
// bits of the plain call followed by slm_silu_mul.  SLM_MOE_SILU_MUL | SLM_MOE_QUANT_OUT: the gate wave does not store
// T; its T-rounded 32 x 32 tile is exactly one MX block per row, and it writes that block as the down GEMM's input:
// 16 code bytes cq[idx, tile * 16 ..] and the byte c_scale[idx, tile].  A row's 32 columns sit in lanes m and m + 32,
// four registers of packed pairs each: the packed-u16 amax crosses the halves once, then each lane trades two of its
// four registers for the partner's, which leaves lane half h with the 16 consecutive columns 16 h .. 16 h + 15 = ONE
// 8-byte store.  amax, exponent and convert are w4a4_quant.h's own functions on the same T bits: the result is
// slm_w4a4_quantize_act on the SLM_MOE_SILU_MUL output byte for byte (-0 codes and scale bytes included).
// Padding rows are never stored.  No split-K, no workspace, no atomics.
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include <type_traits>

#include "common.h"
#include "moe_gemm_plan.h"
#include "w4a4_quant.h"

namespace slm {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int MW4_RING = 3;                // weight / A register rings (chunks), w4a4.hip's
constexpr int MW4_CODES = 32 * 64;         // bytes of a stage's code image; the scale bytes follow
constexpr int MW4_STAGE = MW4_CODES + 32 * 4;

struct MoeW4A4KParams {
  const char* a;            // [n_flat / a_div, K / 2] code bytes
  const uint8_t* a_scale;   // [n_flat / a_div, K / 32] e8m0 bytes
  const char* w;            // expert 0
  const uint8_t* w_scale;   // expert 0's [N, K / 32] e8m0 bytes
  void* c;                  // T, or with quant the code bytes
  uint8_t* c_scale;         // quant: [n_flat, N / 64]
  const float* row_scale;   // [n_flat] or NULL
  const int32_t* sorted;    // [>= n_padded]
  const int32_t* expert_ids;
  const int32_t* n_padded;  // [1]
  int64_t w_stride;         // bytes per expert
  int64_t scale_stride;     // scale bytes per expert
  int64_t lda, ldas, ldw, lds;  // bytes
  int64_t ldc;              // elements of T; quant: bytes
  int64_t ldcs;             // bytes
  int n_flat;               // rows of c; indices >= n_flat are padding
  int a_div;
  int n_experts;
  int n_tiles;              // N / 32
  int n_chunks;             // K / 128
  int tail_units;           // (K % 128) / 32
  int n_nblocks;            // workgroups per row block
  int silu;
  int quant;
};

// D = A . B + C over 64 k: e2m1 codes of one MX block per lane and operand, their e8m0 bytes in byte 0 of sa / sb
__device__ __forceinline__ f32x16 mw4_mfma(const u32x4 a, const uint32_t sa, const u32x4 b, const uint32_t sb,
                                           const f32x16 c) {
  const i32x8 av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
  const i32x8 bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, 4, 4, 0, (int)sa, 0, (int)sb);
}

template <typename T, int NW>
__global__ void __launch_bounds__(NW * 64) moe_w4a4_kernel(const MoeW4A4KParams p) {
  constexpr int RING = MW4_RING;
  constexpr int NT = NW * 64;
  constexpr int NBLK = 128;                     // MX blocks of a chunk of the block's 32 rows
  constexpr int P = (NBLK + NT - 1) / NT;       // ... per thread
  constexpr int CODES = MW4_CODES, STAGE = MW4_STAGE;
  static_assert(STAGE % 16 == 0 && 2 * STAGE >= (NW / 2) * 4 * 64 * 8, "the SiLU exchange fits the stages");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  __shared__ int s_idx[32];  // the block's flat indices, for the scatter in the epilogue
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nb = blockIdx.x % p.n_nblocks;
  const int mb = blockIdx.x / p.n_nblocks;
  if ((int64_t)mb * 32 >= (int64_t)p.n_padded[0]) return;  // beyond the aligned list: nothing to do
  const int e = p.expert_ids[mb];
  if ((unsigned)e >= (unsigned)p.n_experts) return;        // never produced by the align step

  // ---- the wave's column tile (moe_gemm.hip) ----
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

  // ---- A: this thread's P blocks (row, blk) of a chunk; the row comes from the sorted list ----
  const int32_t* sblk = p.sorted + (int64_t)mb * 32;
  if (tid < 32) s_idx[tid] = sblk[tid];
  const char* a_src[P];
  const uint8_t* as_src[P];
  int a_dst[P], as_dst[P];
  bool a_own[P];
  int a_blk[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int b = tid + NT * i;
    a_own[i] = b < NBLK;
    const int row = (b >> 2) & 31, blk = b & 3;
    const int fi = sblk[row];
    const int64_t ar = (unsigned)fi < (unsigned)p.n_flat ? fi / p.a_div : 0;  // padding: a clamped row
    a_blk[i] = blk;
    a_src[i] = p.a + ar * p.lda + blk * 16;
    as_src[i] = p.a_scale + ar * p.ldas + blk;
    a_dst[i] = row * 64 + ((blk ^ ((row >> 2) & 3)) << 4);
    as_dst[i] = CODES + row * 4 + blk;
  }
  // lane half kh: blocks 2 kh, 2 kh + 1 of the chunk = 32 contiguous bytes of row n of expert e, and their scale bytes
  const int64_t wrow = (int64_t)nt * 32 + mrow;
  const char* wlane = p.w + (int64_t)e * p.w_stride + wrow * p.ldw;
  const uint8_t* slane = p.w_scale + (int64_t)e * p.scale_stride + wrow * p.lds;
  uint32_t one = 1;
  asm("" : "+s"(one));  // an opaque offset: the two byte loads are not merged into one 2-byte load (dense.hip)
  const uint8_t* slane1 = slane + one;
  const int f_off = mrow * 64;            // the row's codes
  const int f_swz = (mrow >> 2) & 3;
  const int fs_off = CODES + mrow * 4;    // the row's scale bytes

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  const int nC = p.n_chunks;
  if (nC > 0) {
    const int last = nC - 1;
    auto clampc = [&](int c) { return c < last ? c : last; };
    u32x4 areg[RING][P];
    uint32_t asreg[RING][P];
    u32x4 wreg[RING][2];
    uint32_t sreg[RING][2];
    auto a_load = [&](int c, u32x4 (&dst)[P], uint32_t (&s)[P]) {
      const uint32_t cc = (uint32_t)clampc(c);
#pragma unroll
      for (int i = 0; i < P; ++i) {
        if (a_own[i]) {
          dst[i] = *reinterpret_cast<const u32x4*>(a_src[i] + cc * 64u);
          s[i] = as_src[i][cc * 4u];
        }
      }
    };
    auto a_store = [&](int stage, const u32x4 (&src)[P], const uint32_t (&s)[P]) {
#pragma unroll
      for (int i = 0; i < P; ++i) {
        if (a_own[i]) {
          *reinterpret_cast<u32x4*>(smem + stage * STAGE + a_dst[i]) = src[i];
          *reinterpret_cast<uint8_t*>(smem + stage * STAGE + as_dst[i]) = (uint8_t)s[i];
        }
      }
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
            const u32x4 af = *reinterpret_cast<const u32x4*>(sbase + f_off + ((blk ^ f_swz) << 4));
            const uint32_t asc = *reinterpret_cast<const uint8_t*>(sbase + fs_off + blk);
            acc = mw4_mfma(wreg[u][j], sreg[u][j], af, asc, acc);
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

  // ---- K % 128: up to three blocks, step s gives lane half kh the unit 2 s + kh ----
  if (p.tail_units > 0) {
    __syncthreads();  // nC == 0: s_idx; otherwise nobody reads the stages any more
#pragma unroll
    for (int i = 0; i < P; ++i) {
      if (a_own[i] && a_blk[i] < p.tail_units) {
        *reinterpret_cast<u32x4*>(smem + a_dst[i]) = *reinterpret_cast<const u32x4*>(a_src[i] + (uint32_t)nC * 64u);
        *reinterpret_cast<uint8_t*>(smem + as_dst[i]) = as_src[i][(uint32_t)nC * 4u];
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (2 * s < p.tail_units) {
        const int unit = 2 * s + kh;
        const bool live = unit < p.tail_units;
        const int uu = live ? unit : 0;  // a lane without a unit: zero codes, loads stay inside the row
        u32x4 wv = *reinterpret_cast<const u32x4*>(wlane + (uint32_t)nC * 64u + uu * 16);
        uint32_t wsc = slane[(uint32_t)nC * 4u + uu];
        u32x4 af = *reinterpret_cast<const u32x4*>(smem + f_off + ((uu ^ f_swz) << 4));
        uint32_t asc = *reinterpret_cast<const uint8_t*>(smem + fs_off + uu);
        if (!live) { wv = u32x4{0, 0, 0, 0}; wsc = 127; af = u32x4{0, 0, 0, 0}; asc = 127; }
        acc = mw4_mfma(wv, wsc, af, asc, acc);
      }
    }
  }
  __syncthreads();  // the SiLU exchange below reuses the stages

  // ---- epilogue.  C^T layout: lane (m = lane & 31, kh) holds row m of the block, registers 4 j .. 4 j + 3 = columns
  // 8 j + 4 kh + {0..3} of the tile.  s_idx was written before the first barrier
  const int fi = s_idx[mrow];
  const bool live_row = (unsigned)fi < (unsigned)p.n_flat;
  const int ncol0 = nt * 32 + 4 * kh;  // + 8 j
  uint16_t* cbase = reinterpret_cast<uint16_t*>(p.c);
  float rs = 1.f;
  if (p.row_scale && live_row) rs = p.row_scale[fi];
  u32x2 packed[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p.row_scale) {
      packed[j].x = pack2<T>(acc[4 * j] * rs, acc[4 * j + 1] * rs);
      packed[j].y = pack2<T>(acc[4 * j + 2] * rs, acc[4 * j + 3] * rs);
    } else {
      packed[j].x = pack2<T>(acc[4 * j], acc[4 * j + 1]);
      packed[j].y = pack2<T>(acc[4 * j + 2], acc[4 * j + 3]);
    }
  }
  if constexpr (NW >= 2) {
    if (p.silu) {
      // the up wave hands its T-rounded tile to the gate wave through the (now idle) stages; same lane, same j
      u32x2* ex = reinterpret_cast<u32x2*>(smem) + (wave >> 1) * (4 * 64);
      if (wave & 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ex[j * 64 + lane] = packed[j];
      }
      __syncthreads();
      if ((wave & 1) || !nvalid) return;
      u32x2 r[4];  // the gate wave: nt = the output tile
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32x2 g = packed[j], u = ex[j * 64 + lane];
        r[j].x = pack2<T>(silu_mul1(lo_f32<T>(g.x), lo_f32<T>(u.x)), silu_mul1(hi_f32<T>(g.x), hi_f32<T>(u.x)));
        r[j].y = pack2<T>(silu_mul1(lo_f32<T>(g.y), lo_f32<T>(u.y)), silu_mul1(hi_f32<T>(g.y), hi_f32<T>(u.y)));
      }
      if (!p.quant) {
        if (live_row) {
#pragma unroll
          for (int j = 0; j < 4; ++j) *reinterpret_cast<u32x2*>(cbase + (int64_t)fi * p.ldc + ncol0 + 8 * j) = r[j];
        }
        return;
      }
      // the tile's row as one MX block (all 64 lanes take part in the exchanges: padding rows are only kept from
      // storing)
      uint32_t e8;
      const u32x2 codes = quantize_tile_row<T>(r, kh, e8);
      if (live_row) {
        *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(p.c) + (int64_t)fi * p.ldc + nt * 16 + kh * 8) = codes;
        if (kh == 0) p.c_scale[(int64_t)fi * p.ldcs + nt] = (uint8_t)e8;
      }
      return;
    }
  }
  if (!nvalid || !live_row) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) *reinterpret_cast<u32x2*>(cbase + (int64_t)fi * p.ldc + ncol0 + 8 * j) = packed[j];
}

// ---- host ----
template <typename T>
static void launch_moe_w4a4(const MoeW4A4KParams& kp, int nw, unsigned grid, hipStream_t st) {
  if (nw == 4) hipLaunchKernelGGL((moe_w4a4_kernel<T, 4>), dim3(grid), dim3(256), 0, st, kp);
  else if (nw == 2) hipLaunchKernelGGL((moe_w4a4_kernel<T, 2>), dim3(grid), dim3(128), 0, st, kp);
  else hipLaunchKernelGGL((moe_w4a4_kernel<T, 1>), dim3(grid), dim3(64), 0, st, kp);
}

static int run_moe_w4a4(const slm_moe_w4a4_gemm_args* a, void* stream) {
  if (!a) return SLM_ERR_INVALID_ARG;
  if (a->n_flat < 0 || a->K <= 0 || a->N <= 0 || a->a_div < 1 || a->n_experts < 1 || a->max_blocks < 0)
    return SLM_ERR_INVALID_ARG;
  if (a->dtype != SLM_F16 && a->dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (a->flags & ~(SLM_MOE_SILU_MUL | SLM_MOE_QUANT_OUT)) return SLM_ERR_INVALID_ARG;
  const bool silu = (a->flags & SLM_MOE_SILU_MUL) != 0;
  const bool quant = (a->flags & SLM_MOE_QUANT_OUT) != 0;
  if (quant && !silu) return SLM_ERR_INVALID_ARG;
  if (silu && a->row_scale) return SLM_ERR_INVALID_ARG;
  if (a->K % 32 || a->N % 32 || (silu && (a->N / 2) % 32)) return SLM_ERR_UNSUPPORTED;
  // 32-bit byte offsets inside one expert; flat indices are int32
  const int64_t krow = a->K / 2, kblk = a->K / 32;
  if (krow * a->N >= ((int64_t)1 << 32) || a->n_flat >= ((int64_t)1 << 31) - 256) return SLM_ERR_UNSUPPORTED;
  if (a->n_flat == 0 || a->max_blocks == 0) return SLM_OK;
  if (!a->a || !a->a_scale || !a->w || !a->w_scale || !a->c || (quant && !a->c_scale) || !a->sorted_token_idxes ||
      !a->expert_ids || !a->n_padded_tokens)
    return SLM_ERR_INVALID_ARG;
  // c: [n_flat, N] T, SiLU [n_flat, N / 2] T, quantised [n_flat, N / 4] bytes + [n_flat, N / 64] scale bytes
  const int64_t n_out = quant ? a->N / 4 : silu ? a->N / 2 : a->N;
  if (a->lda < krow || a->ldas < kblk || a->ldw < krow || a->ldc < n_out || (quant && a->ldcs < a->N / 64) ||
      a->w_expert_stride < (a->N - 1) * a->ldw + krow || a->lds < kblk ||
      a->w_scale_expert_stride < (a->N - 1) * a->lds + kblk)
    return SLM_ERR_INVALID_ARG;
  // 16-byte loads of A and W; 8-byte stores of C (T: four elements; quantised: 16 codes)
  if (!aligned16(a->a) || a->lda % 16 || !aligned16(a->w) || a->ldw % 16 || a->w_expert_stride % 16 ||
      (quant ? !aligned16(a->c) || a->ldc % 16 : (reinterpret_cast<uintptr_t>(a->c) & 7u) || a->ldc % 4) ||
      (reinterpret_cast<uintptr_t>(a->row_scale) & 3u))
    return SLM_ERR_ALIGNMENT;
  if (a->N * a->ldw >= ((int64_t)1 << 32) || a->N * a->lds >= ((int64_t)1 << 32)) return SLM_ERR_UNSUPPORTED;
  const int64_t n_tiles = a->N / 32;
  const int nw = moe_gemm_waves(a->max_blocks, n_tiles, silu);
  const int64_t n_nblocks = gemm_col_groups(n_tiles, nw, silu);
  const int64_t grid = (int64_t)a->max_blocks * n_nblocks;
  if (grid >= ((int64_t)1 << 31)) return SLM_ERR_UNSUPPORTED;

  MoeW4A4KParams kp;
  kp.a = reinterpret_cast<const char*>(a->a);
  kp.a_scale = a->a_scale;
  kp.w = reinterpret_cast<const char*>(a->w);
  kp.w_scale = a->w_scale;
  kp.c = a->c;
  kp.c_scale = quant ? a->c_scale : nullptr;
  kp.row_scale = a->row_scale;
  kp.sorted = a->sorted_token_idxes;
  kp.expert_ids = a->expert_ids;
  kp.n_padded = a->n_padded_tokens;
  kp.w_stride = a->w_expert_stride;
  kp.scale_stride = a->w_scale_expert_stride;
  kp.lda = a->lda; kp.ldas = a->ldas; kp.ldw = a->ldw; kp.lds = a->lds; kp.ldc = a->ldc; kp.ldcs = a->ldcs;
  kp.n_flat = (int)a->n_flat;
  kp.a_div = a->a_div;
  kp.n_experts = a->n_experts;
  kp.n_tiles = (int)n_tiles;
  kp.n_chunks = (int)(a->K / MG_KC);
  kp.tail_units = (int)((a->K % MG_KC) / 32);
  kp.n_nblocks = (int)n_nblocks;
  kp.silu = silu ? 1 : 0;
  kp.quant = quant ? 1 : 0;
  hip_clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dispatch_dtype(a->dtype, [&](auto t) { launch_moe_w4a4<decltype(t)>(kp, nw, (unsigned)grid, st); });
  return hip_check_launch();
}

}  // namespace slm

extern "C" {

SLM_API int slm_moe_w4a4_gemm(const slm_moe_w4a4_gemm_args* a, void* stream) { return slm::run_moe_w4a4(a, stream); }

}  // extern "C"
