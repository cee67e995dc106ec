// w8a8_moe.hip -- grouped fp8 x fp8 GEMM over the experts of a mixture-of-experts layer on the 32x32x64 fp8 MFMA
// (include/slm_hip.h section 26, slm_moe_w8a8_gemm): moe_gemm.hip's aligned-list contract with w8a8.hip's arithmetic.
//
// For every 32-row block b of the aligned token list (slm_moe_align_block with block_size 32), e = expert_ids[b],
// idx = sorted[b * 32 + r], m = idx / a_div:
//     acc       = sum_k e4m3(Aq[m, k]) * e4m3(W_e[n, k])        fp32, every product exact
//     y         = (acc * a_scale[m]) * w_scale[e, n]            two fp32 multiplies, this order, uncontracted
//     C[idx, n] = T( y * row_scale[idx] )                       one rounding
// The experts are section 16's checkpoint tensors ([E, N, K] e4m3 bytes, [E, N] fp32 channel scales), the activations
// are PRE-QUANTISED (slm_w8a8_quantize_act, once per token: the rule is per row, so it commutes with the gather
// idx / a_div).  There is no T side: a per-token scale needs the whole row before the first byte can be converted.
//
// One wave, one tile (w4a4_moe.hip's split).  A wave owns one 32 x 32 output tile over the whole K; a workgroup is
// NW = 4 / 2 / 1 waves on adjacent column tiles (SiLU * mul: (gate, up) pairs) sharing the LDS image of the block's 32
// gathered rows; the host takes moe_gemm_waves(max_blocks, n_tiles, silu).  The wave's MFMA sequence over k is
// w8a8_linear_kernel's at RT = 1 and split_k = 1, statement for statement: weights are MFMA operand A, activations
// operand B (the accumulator is the C^T tile: lane (m = lane & 31, h = lane >> 5) holds row m, registers 4 j .. 4 j + 3
// = columns 8 j + 4 h + {0..3}); K in 128-deep chunks of four 32-byte units, TWO v_mfma_f32_32x32x64_f8f6f4 per chunk
// and ZERO converts, step j giving lane half h the unit 2 h + j on both operands -- a lane's weights of a chunk are 64
// contiguous bytes of row n of expert e: four 16-B loads, held in a 3-chunk register ring refilled right after its
// MFMAs; K % 128 in steps of natural order (step s: unit 2 s + h), a lane without a unit feeding zero bytes (e4m3 0x00
// = +0) on both operands.  So no result bit depends on NW, and an expert's rows are slm_w8a8_linear
// (SLM_W8A8_SPLITK = 1) on those rows bit for bit.  The loop is written out here and not shared with w8a8.hip through a
// header: w4a4.hip's loop moved into a forceinline function cost its RT = 4 forms 60 VGPRs, and
// w8a8.hip's forms sit at up to 170; w8a8.hip stays byte for byte as it is.
//
// A through LDS.  A chunk's image is w8a8.hip's at one row tile: [32 rows][8 slots] x 16 B (slot XOR (row >> 1 & 7))
// = 4096 B, double buffered.  Each of the chunk's 256 slots has ONE owner thread in the workgroup (NW = 4: one per
// thread, NW = 1: four), which copies 16 B of the gathered row; the owner's ring is stored to the other buffer one
// iteration before its use.  One barrier per chunk (two MFMAs).
//
// Addresses.  Dead blocks (beyond n_padded) and expert ids outside [0, E) leave before any address is formed.  Row n =
// nt * 32 + (lane & 31) < N because nt is clamped to a valid tile.  A ring load of chunk c reads bytes
// [128 cc + 64 h, + 64) of the row with cc = min(c, n_chunks - 1): below 128 n_chunks <= K; a tail load reads
// [128 n_chunks + 32 u, + 32) with u < tail_units: below K.  The host checks ldw >= K and w_expert_stride >=
// (N - 1) * ldw + K: no byte outside expert e's own [N, K] rows is read, whatever the padding holds.  w_scale is read
// at e * w_scale_expert_stride + n, n < N.  A: a padding id (>= n_flat) is clamped to row 0, a live one reads row
// idx / a_div (64-bit row offset), bytes [128 cc + 16 slot, + 16) under the same clamp, the tail [128 n_chunks +
// 16 slot, + 16) for slot < 2 tail_units: below K <= lda.  a_scale is read at idx / a_div of live rows only.
//
// Epilogue.  a_scale and w_scale are read once each, here; y * row_scale is a third fp32 multiply, then one rounding
// and 8-byte stores (C 8-byte aligned, ldc % 4 == 0).  SLM_MOE_SILU_MUL: w8a8.hip's -- the up wave hands its T-rounded
// tile to the gate wave through the idle stages: the bits of the plain call followed by slm_silu_mul.  Padding rows
// are never stored.  No split-K, no workspace, no atomics.  (The sign of a zero: w8a8.hip adds its bias operand, 0.0
// without one, so a sum that is exactly zero under a NEGATIVE scale leaves it as +0 and this file as -0; checkpoints'
// scales are positive.)
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include <type_traits>

#include "common.h"
#include "fp8_cvt.h"
#include "moe_gemm_plan.h"

namespace slm {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int MW8_RING = 3;          // weight / A register rings (chunks), w8a8.hip's
constexpr int MW8_STAGE = 32 * 128;  // bytes of a stage: 32 rows x 128 k

struct MoeW8A8KParams {
  const char* a;            // [n_flat / a_div, K] e4m3 bytes
  const float* a_scale;     // [n_flat / a_div] or NULL (1.0)
  const char* w;            // expert 0
  const float* w_scale;     // expert 0's [N] channel scales, or NULL (1.0)
  void* c;
  const float* row_scale;   // [n_flat] or NULL
  const int32_t* sorted;    // [>= n_padded]
  const int32_t* expert_ids;
  const int32_t* n_padded;  // [1]
  int64_t w_stride;         // bytes per expert
  int64_t scale_stride;     // floats per expert
  int64_t lda, ldw;         // bytes
  int64_t ldc;              // elements of T
  int n_flat;               // rows of c; indices >= n_flat are padding
  int a_div;
  int n_experts;
  int n_tiles;              // N / 32
  int n_chunks;             // K / 128
  int tail_units;           // (K % 128) / 32
  int n_nblocks;            // workgroups per row block
  int silu;
};

// D = A . B + C over 64 k: 32 e4m3 bytes per lane and operand (w8a8.hip's mfma_f8)
__device__ __forceinline__ f32x16 mw8_mfma(const u32x4 a0, const u32x4 a1, const u32x4 b0, const u32x4 b1,
                                           const f32x16 c) {
  const i32x8 av = {(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
  const i32x8 bv = {(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, 0, 0, 0, 0, 0, 0);
}

template <typename T, int NW>
__global__ void __launch_bounds__(NW * 64) moe_w8a8_kernel(const MoeW8A8KParams p) {
  constexpr int RING = MW8_RING;
  constexpr int NT = NW * 64;
  constexpr int NSLOT = 32 * 8;     // 16-B slots of a chunk of the block's 32 rows
  constexpr int P = NSLOT / NT;     // ... per thread
  constexpr int STAGE = MW8_STAGE;
  static_assert(NSLOT % NT == 0 && P >= 1 && P <= 4, "one owner per slot");
  static_assert(2 * STAGE >= (NW / 2) * 4 * 64 * 8, "the SiLU exchange fits the stages");
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

  // ---- A: this thread's P slots (row, slot) of a chunk; the row comes from the sorted list ----
  const int32_t* sblk = p.sorted + (int64_t)mb * 32;
  if (tid < 32) s_idx[tid] = sblk[tid];
  const char* a_src[P];
  int a_dst[P];
  const int a_slot = tid & 7;  // NT % 8 == 0: the same slot in every one of the thread's rows
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int row = (tid + NT * i) >> 3;
    const int fi = sblk[row];
    const int64_t ar = (unsigned)fi < (unsigned)p.n_flat ? fi / p.a_div : 0;  // padding: a clamped row
    a_src[i] = p.a + ar * p.lda + a_slot * 16;
    a_dst[i] = row * 128 + ((a_slot ^ ((row >> 1) & 7)) << 4);
  }
  // lane half kh: units 2 kh, 2 kh + 1 of the chunk = 64 contiguous bytes of row n of expert e
  const int64_t wrow = (int64_t)nt * 32 + mrow;
  const char* wlane = p.w + (int64_t)e * p.w_stride + wrow * p.ldw;
  const int f_off = mrow * 128;  // the row's bytes
  const int f_swz = (mrow >> 1) & 7;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  const int nC = p.n_chunks;
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
            const u32x4 af0 = *reinterpret_cast<const u32x4*>(sbase + ((slot ^ f_swz) << 4));
            const u32x4 af1 = *reinterpret_cast<const u32x4*>(sbase + (((slot + 1) ^ f_swz) << 4));
            acc = mw8_mfma(wreg[u][2 * j], wreg[u][2 * j + 1], af0, af1, acc);
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

  // ---- K % 128: up to three units, step s gives lane half kh the unit 2 s + kh ----
  if (p.tail_units > 0) {
    __syncthreads();  // nC == 0: s_idx; otherwise nobody reads the stages any more
    if ((a_slot >> 1) < p.tail_units) {
#pragma unroll
      for (int i = 0; i < P; ++i)
        *reinterpret_cast<u32x4*>(smem + a_dst[i]) = *reinterpret_cast<const u32x4*>(a_src[i] + (uint32_t)nC * 128u);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (2 * s < p.tail_units) {
        const int unit = 2 * s + kh;
        const bool live = unit < p.tail_units;
        const int uu = live ? unit : 0;  // a lane without a unit: zero bytes, loads stay inside the row
        const char* wsrc = wlane + (uint32_t)nC * 128u + uu * 32;
        u32x4 w0 = *reinterpret_cast<const u32x4*>(wsrc);
        u32x4 w1 = *reinterpret_cast<const u32x4*>(wsrc + 16);
        u32x4 af0 = *reinterpret_cast<const u32x4*>(smem + f_off + (((2 * uu) ^ f_swz) << 4));
        u32x4 af1 = *reinterpret_cast<const u32x4*>(smem + f_off + (((2 * uu + 1) ^ f_swz) << 4));
        if (!live) { w0 = u32x4{0, 0, 0, 0}; w1 = w0; af0 = w0; af1 = w0; }
        acc = mw8_mfma(w0, w1, af0, af1, acc);
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
  float as = 1.f, rs = 1.f;
  if (p.a_scale && live_row) as = p.a_scale[fi / p.a_div];
  if (p.row_scale && live_row) rs = p.row_scale[fi];
  const float* wsc = p.w_scale ? p.w_scale + (int64_t)e * p.scale_stride + ncol0 : nullptr;
  u32x2 packed[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // y = (acc * a_scale[m]) * w_scale[e, n]
      const float s = wsc ? wsc[8 * j + i] : 1.f;
      y[i] = scaled(scaled(acc[4 * j + i], as), s);
    }
    if (p.row_scale) {
      packed[j].x = pack2<T>(y[0] * rs, y[1] * rs);
      packed[j].y = pack2<T>(y[2] * rs, y[3] * rs);
    } else {
      packed[j].x = pack2<T>(y[0], y[1]);
      packed[j].y = pack2<T>(y[2], y[3]);
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
      if ((wave & 1) || !nvalid || !live_row) return;
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // the gate wave: nt = the output tile
        const u32x2 g = packed[j], u = ex[j * 64 + lane];
        u32x2 r;
        r.x = pack2<T>(silu_mul1(lo_f32<T>(g.x), lo_f32<T>(u.x)), silu_mul1(hi_f32<T>(g.x), hi_f32<T>(u.x)));
        r.y = pack2<T>(silu_mul1(lo_f32<T>(g.y), lo_f32<T>(u.y)), silu_mul1(hi_f32<T>(g.y), hi_f32<T>(u.y)));
        *reinterpret_cast<u32x2*>(cbase + (int64_t)fi * p.ldc + ncol0 + 8 * j) = r;
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
static void launch_moe_w8a8(const MoeW8A8KParams& kp, int nw, unsigned grid, hipStream_t st) {
  if (nw == 4) hipLaunchKernelGGL((moe_w8a8_kernel<T, 4>), dim3(grid), dim3(256), 0, st, kp);
  else if (nw == 2) hipLaunchKernelGGL((moe_w8a8_kernel<T, 2>), dim3(grid), dim3(128), 0, st, kp);
  else hipLaunchKernelGGL((moe_w8a8_kernel<T, 1>), dim3(grid), dim3(64), 0, st, kp);
}

// section 16's rules (moe_gemm.hip: run_moe_gemm, the fp8 side), rule for rule and in its order; a in bytes, c stored
// 8 bytes at a time
static int run_moe_w8a8(const slm_moe_w8a8_gemm_args* a, void* stream) {
  if (!a) return SLM_ERR_INVALID_ARG;
  if (a->n_flat < 0 || a->K <= 0 || a->N <= 0 || a->a_div < 1 || a->n_experts < 1 || a->max_blocks < 0)
    return SLM_ERR_INVALID_ARG;
  if (a->dtype != SLM_F16 && a->dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (a->flags & ~SLM_MOE_SILU_MUL) return SLM_ERR_INVALID_ARG;
  const bool silu = (a->flags & SLM_MOE_SILU_MUL) != 0;
  if (silu && a->row_scale) return SLM_ERR_INVALID_ARG;
  if (a->K % 32 || a->N % 32 || (silu && (a->N / 2) % 32)) return SLM_ERR_UNSUPPORTED;
  // 32-bit byte offsets inside one expert; flat indices are int32
  if (a->K * a->N >= ((int64_t)1 << 32) || a->n_flat >= ((int64_t)1 << 31) - 256) return SLM_ERR_UNSUPPORTED;
  if (a->n_flat == 0 || a->max_blocks == 0) return SLM_OK;
  if (!a->a || !a->w || !a->c || !a->sorted_token_idxes || !a->expert_ids || !a->n_padded_tokens)
    return SLM_ERR_INVALID_ARG;
  const int64_t n_out = silu ? a->N / 2 : a->N;
  if (a->lda < a->K || a->ldw < a->K || a->ldc < n_out || a->w_expert_stride < (a->N - 1) * a->ldw + a->K)
    return SLM_ERR_INVALID_ARG;
  if (a->w_scale && a->w_scale_expert_stride < a->N) return SLM_ERR_INVALID_ARG;
  // 16-byte loads of A and W; 8-byte stores of C (four elements of T)
  if (!aligned16(a->a) || a->lda % 16 || !aligned16(a->w) || a->ldw % 16 || a->w_expert_stride % 16 ||
      (reinterpret_cast<uintptr_t>(a->c) & 7u) || a->ldc % 4 || (reinterpret_cast<uintptr_t>(a->row_scale) & 3u) ||
      (reinterpret_cast<uintptr_t>(a->w_scale) & 3u) || (reinterpret_cast<uintptr_t>(a->a_scale) & 3u))
    return SLM_ERR_ALIGNMENT;
  if (a->N * a->ldw >= ((int64_t)1 << 32)) return SLM_ERR_UNSUPPORTED;  // a strided expert: still < 4 GiB
  const int64_t n_tiles = a->N / 32;
  const int nw = moe_gemm_waves(a->max_blocks, n_tiles, silu);
  const int64_t n_nblocks = gemm_col_groups(n_tiles, nw, silu);
  const int64_t grid = (int64_t)a->max_blocks * n_nblocks;
  if (grid >= ((int64_t)1 << 31)) return SLM_ERR_UNSUPPORTED;

  MoeW8A8KParams kp;
  kp.a = reinterpret_cast<const char*>(a->a);
  kp.a_scale = a->a_scale;
  kp.w = reinterpret_cast<const char*>(a->w);
  kp.w_scale = a->w_scale;
  kp.c = a->c;
  kp.row_scale = a->row_scale;
  kp.sorted = a->sorted_token_idxes;
  kp.expert_ids = a->expert_ids;
  kp.n_padded = a->n_padded_tokens;
  kp.w_stride = a->w_expert_stride;
  kp.scale_stride = a->w_scale ? a->w_scale_expert_stride : 0;
  kp.lda = a->lda; kp.ldw = a->ldw; kp.ldc = a->ldc;
  kp.n_flat = (int)a->n_flat;
  kp.a_div = a->a_div;
  kp.n_experts = a->n_experts;
  kp.n_tiles = (int)n_tiles;
  kp.n_chunks = (int)(a->K / MG_KC);
  kp.tail_units = (int)((a->K % MG_KC) / 32);
  kp.n_nblocks = (int)n_nblocks;
  kp.silu = silu ? 1 : 0;
  hip_clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dispatch_dtype(a->dtype, [&](auto t) { launch_moe_w8a8<decltype(t)>(kp, nw, (unsigned)grid, st); });
  return hip_check_launch();
}

}  // namespace slm

extern "C" {

SLM_API int slm_moe_w8a8_gemm(const slm_moe_w8a8_gemm_args* a, void* stream) { return slm::run_moe_w8a8(a, stream); }

}  // extern "C"
