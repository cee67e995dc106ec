// dense.hip -- unquantised f16 / bf16 linear over checkpoint-layout weights (include/slm_hip.h section 13,
// slm_linear; the reference's {Column,Row}ParallelLinearImpl::forward = F::linear, src/layers/linear/
// parallel_linear.cpp):   C[M, N] = T( A[M, K] . W[N, K]^T + bias[N] ).
//
// The weight stream is moe_gemm.hip's: W[n, :] is k-contiguous and that IS an operand of the 32x32x16 MFMA
// (lane (n = lane & 31, h = lane >> 5) holds 8 consecutive k of row n), so the weights go from global memory
// to the MFMA in 16-B loads: no LDS stage, no transpose, no prepack.  K is streamed in 128-deep chunks, lane
// half h takes k = [64 h, 64 h + 64) of the chunk (128 contiguous bytes of row n); A's fragments come from a
// [rows][128 k] LDS image of the chunk in natural k order with w4_stream32.h's XOR swizzle.  A K that is no
// multiple of 128 ends in up to three 32-deep units in natural order.
//
// What differs from the grouped kernel:
//  * RT = 1 / 2 / 4 accumulator tiles of 32 rows per wave: every 16-B weight fragment feeds RT MFMAs, so the
//    weights are streamed once for M <= 32 RT.  More rows go to further row blocks of the grid (blockIdx.z),
//    which stream the weights again: correct, not tuned (prefill is not this kernel's job).
//  * the operands are swapped (weights = MFMA A, activations = MFMA B): the accumulator tile is C^T, lane
//    (m = lane & 31, h) holds for row m the columns 8 j + 4 h + {0..3} in registers 4 j .. 4 j + 3 -- four
//    consecutive columns, stored as ONE 16-B fp32 (slab) or 8-B T store.
//  * K split: blockIdx.y = slice s works on chunks [slice_chunk[s], slice_chunk[s + 1]) (the tail units go
//    with the last slice) and writes the fp32 slab s of [split_k][M][N] with plain stores; the reduce kernel
//    (or a deferred consumer: slm_rms_norm_splitk, slm_rope_kv_append_splitk, slm_gemma_norm) sums the slabs
//    with splitk_sum4 in slice order.  No atomics, no flags, no cross-workgroup hand-off.
//  * bias, and SiLU * mul over gate | up rows as in moe_gemm.hip (waves (0, 1) and (2, 3) hold the gate and
//    up tiles of one output tile; the up wave hands its T-rounded tile over through LDS).
//
// A workgroup is NW = 1 / 2 / 4 waves on adjacent column tiles sharing the A image; NW >= RT keeps the A
// ring at <= 8 16-B pieces per thread and chunk (the register budget of the three-chunk ring).  The host takes
// the narrowest NW that leaves at most two workgroups per CU; a wave's arithmetic does not depend on NW or RT.
// A partial last row tile clamps the row on load and suppresses the store; a partial NW group duplicates the
// last column tile and does not store it.
//
// Pipeline (moe_gemm.hip's): weights in a 3-chunk register ring, refilled right after their MFMAs; A in a
// 3-chunk register ring, written to the other LDS buffer one iteration before its use.  VMEM completes in
// order, so the A chunk that is waited for is two iterations old and the wait leaves two weight chunks in
// flight.  Loads past the slice's last chunk are clamped to it and never used.
#include "common.h"
#include "tuning.h"

namespace slm {

constexpr int LIN_RING = 3;   // weight / A register rings (chunks)
constexpr int LIN_KC = 128;   // k per chunk
constexpr int LIN_MAX_SPLIT = 16;

struct LinearKParams {
  const char* a;
  const char* w;
  const void* bias;  // [N] T or NULL
  void* c;
  float* part;       // [split_k][M][N] or NULL (split_k == 1)
  int64_t lda, ldw, ldc;  // elements
  int M, N;
  int n_tiles;       // N / 32
  int tail_units;    // (K % 128) / 32
  int split_k;
  int silu;
  int slice_chunk[LIN_MAX_SPLIT + 1];
};

template <typename T, int RT, int NW>
__global__ void __launch_bounds__(NW * 64) linear_kernel(const LinearKParams p) {
  typedef typename Mfma<T>::frag frag_t;
  constexpr int NT = NW * 64;
  constexpr int ROWS = RT * 32;
  constexpr int STAGE = ROWS * 256;  // one chunk of A: ROWS x 128 k
  constexpr int P = ROWS * 16 / NT;  // 16-B pieces of a chunk of A per thread
  static_assert(P >= 1 && P <= 8, "NW >= RT");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nb = blockIdx.x, ks = blockIdx.y;
  const int row0 = blockIdx.z * ROWS;

  // ---- the wave's column tile ----
  int nt;
  bool nvalid;
  if (p.silu) {
    // pairs of waves: (gate, up) tiles of output tile pi
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

  // ---- the slice's chunks ----
  const int c0 = p.slice_chunk[ks];
  const int nC = p.slice_chunk[ks + 1] - c0;
  const int tail_units = ks == p.split_k - 1 ? p.tail_units : 0;
  const uint32_t kbase = (uint32_t)c0 * 256u;  // bytes into a row

  // ---- A: this thread's P (row, 16-B slot) sources of a chunk; rows beyond M are clamped, never stored ----
  const char* a_src[P];
  int a_dst[P];
  const int a_slot = tid & 15;  // NT % 16 == 0: one slot for all of a thread's pieces
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int idx = tid + NT * i;
    const int row = idx >> 4, slot = idx & 15;
    int gr = row0 + row;
    gr = gr < p.M ? gr : p.M - 1;
    a_src[i] = p.a + 2 * ((int64_t)gr * p.lda + slot * 8) + kbase;
    a_dst[i] = stage_swz(row, slot);
  }
  const char* wlane = p.w + 2 * (((int64_t)nt * 32 + mrow) * p.ldw) + kbase;
  const int a_row = mrow * 256;
  const int a_swz = mrow & 15;

  f32x16 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  if (nC > 0) {
    const int last = nC - 1;
    auto clampc = [&](int c) { return c < last ? c : last; };
    u32x4 areg[LIN_RING][P];
    u32x4 wreg[LIN_RING][8];
    auto a_load = [&](int c, u32x4 (&dst)[P]) {
      const uint32_t off = (uint32_t)clampc(c) * 256u;
#pragma unroll
      for (int i = 0; i < P; ++i) dst[i] = *reinterpret_cast<const u32x4*>(a_src[i] + off);
    };
    auto a_store = [&](int stage, const u32x4 (&src)[P]) {
#pragma unroll
      for (int i = 0; i < P; ++i) *reinterpret_cast<u32x4*>(smem + stage * STAGE + a_dst[i]) = src[i];
    };
    // lane half kh: the 128 contiguous bytes [kh * 128, kh * 128 + 128) of the chunk's 256 B of row n
    const char* wl = wlane + kh * 128;
    auto w_load = [&](int c, u32x4 (&w)[8]) {
      const uint32_t off = (uint32_t)clampc(c) * 256u;
#pragma unroll
      for (int q = 0; q < 8; ++q) w[q] = *reinterpret_cast<const u32x4*>(wl + off + q * 16);
    };

    // prologue in the order the steady-state iterations issue (A, then the weights of the same chunk)
    a_load(0, areg[0]);
    w_load(0, wreg[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int d = 1; d < LIN_RING; ++d) {
      a_load(d, areg[d]);
      __builtin_amdgcn_sched_barrier(0);
      w_load(d, wreg[d]);
      __builtin_amdgcn_sched_barrier(0);
    }
    a_store(0, areg[0]);
    __syncthreads();

    int stage = 0;
    const int n_iter = (nC + LIN_RING - 1) / LIN_RING * LIN_RING;
    for (int base = 0; base < n_iter; base += LIN_RING) {
#pragma unroll
      for (int u = 0; u < LIN_RING; ++u) {
        const int i = base + u;  // chunk; ring slot u
        // A for chunk i + 3 into the registers chunk i left (stored one iteration ago)
        a_load(i + LIN_RING, areg[u]);
        __builtin_amdgcn_sched_barrier(0);
        if (i < nC) {
          const char* sbase = smem + stage * STAGE + a_row;
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const frag_t wf = __builtin_bit_cast(frag_t, wreg[u][q]);
#pragma unroll
            for (int t = 0; t < RT; ++t) {
              const frag_t af = __builtin_bit_cast(
                  frag_t, *reinterpret_cast<const u32x4*>(sbase + t * (32 * 256) + (((kh * 8 + q) ^ a_swz) << 4)));
              acc[t] = Mfma<T>::run(wf, af, acc[t]);
            }
          }
        }
        // the refill AFTER the old values are consumed (pinned): each ring slot keeps its registers
        __builtin_amdgcn_sched_barrier(0);
        w_load(i + LIN_RING, wreg[u]);
        __builtin_amdgcn_sched_barrier(0);
        // chunk i + 1 (loaded two iterations ago) -> the buffer everybody finished reading one barrier ago
        a_store(stage ^ 1, areg[(u + 1) % LIN_RING]);
        __syncthreads();
        stage ^= 1;
      }
    }
  }

  // ---- K % 128 (last slice): up to three 32-deep units in natural k order, one at a time ----
  if (tail_units > 0) {
    const uint32_t koff = (uint32_t)nC * 256u;  // bytes behind the slice's chunks
    __syncthreads();                            // nobody reads the stages any more
#pragma unroll
    for (int i = 0; i < P; ++i) {
      if (a_slot < tail_units * 4)
        *reinterpret_cast<u32x4*>(smem + a_dst[i]) = *reinterpret_cast<const u32x4*>(a_src[i] + koff);
    }
    __syncthreads();
    const char* sbase = smem + a_row;
    const char* wt = wlane + koff + kh * 32;
#pragma unroll
    for (int t3 = 0; t3 < 3; ++t3) {
      if (t3 < tail_units) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const frag_t wf = __builtin_bit_cast(frag_t, *reinterpret_cast<const u32x4*>(wt + t3 * 64 + s * 16));
#pragma unroll
          for (int t = 0; t < RT; ++t) {
            const frag_t af = __builtin_bit_cast(
                frag_t, *reinterpret_cast<const u32x4*>(sbase + t * (32 * 256) + (((t3 * 4 + kh * 2 + s) ^ a_swz) << 4)));
            acc[t] = Mfma<T>::run(wf, af, acc[t]);
          }
        }
      }
    }
    __syncthreads();  // the SiLU exchange below reuses the stage
  }

  // ---- epilogue.  C^T layout: lane (m = lane & 31, kh), registers 4 j .. 4 j + 3 = columns 8 j + 4 kh + {0..3}
  const int ncol0 = nt * 32 + 4 * kh;  // + 8 j
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
  // T( acc + bias ), packed pairs
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
      // the up wave hands its T-rounded tiles to the gate wave through the (now idle) A buffers; same lane, same (t, j)
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
            // the gate wave: nt = the output tile
            *reinterpret_cast<u32x2*>(cbase + (int64_t)gm * p.ldc + ncol0 + 8 * j) = r;
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

// ---- the plan: a pure host function of (M, N, K, dtype, flags, bias != NULL, tuning table) ----
struct LinearPlan {
  int rt, nw;
  int64_t row_blocks, col_groups;
  int split_k, n_chunks, tail_units;
  int slice_chunk[LIN_MAX_SPLIT + 1];
  uint64_t lds_bytes, ws_bytes;
};

static int plan_linear(const slm_linear_args* a, LinearPlan* pl) {
  if (!a) return SLM_ERR_INVALID_ARG;
  if (a->M < 0 || a->K <= 0 || a->N <= 0) return SLM_ERR_INVALID_ARG;
  if (a->dtype != SLM_F16 && a->dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (a->flags & ~(SLM_LINEAR_DEFER_REDUCE | SLM_LINEAR_SILU_MUL | SLM_LINEAR_SHARES_CHIP)) return SLM_ERR_INVALID_ARG;
  const bool silu = (a->flags & SLM_LINEAR_SILU_MUL) != 0;
  if (silu && (a->flags & SLM_LINEAR_DEFER_REDUCE)) return SLM_ERR_INVALID_ARG;
  if (a->K % 32 || a->N % 32 || (silu && a->N % 64)) return SLM_ERR_UNSUPPORTED;
  // 32-bit byte offsets inside a row, int rows / columns in the kernel, blockIdx.z row blocks
  if (a->K >= ((int64_t)1 << 30) || a->N >= ((int64_t)1 << 30) || a->M >= ((int64_t)1 << 30)) return SLM_ERR_UNSUPPORTED;

  // row tiles per wave: the fewest of 1 / 2 / 4 that hold all rows (at most 128 per row block)
  int rt = a->M <= 32 ? 1 : a->M <= 64 ? 2 : 4;
  const int rt_knob = tune_get(TUNE_LINEAR_RT, 0);
  if (rt_knob == 1 || rt_knob == 2 || rt_knob == 4) rt = rt_knob;
  const int64_t rows = 32 * rt;
  const int64_t row_blocks = a->M > 0 ? (a->M + rows - 1) / rows : 1;
  if (row_blocks > 65535) return SLM_ERR_UNSUPPORTED;
  const int64_t n_tiles = a->N / 32;
  const int n_chunks = (int)(a->K / LIN_KC);
  // the split the K depth allows: every slice keeps >= 4 chunks
  const int by_depth = n_chunks / 4 < 1 ? 1 : n_chunks / 4 > LIN_MAX_SPLIT ? LIN_MAX_SPLIT : n_chunks / 4;
  // waves per workgroup: the narrowest the form allows (never below the row tiles; SiLU pairs: never below 2),
  // doubled while that leaves more than two workgroups per CU.  Measured at M <= 32 (profiles/r14_dense.jsonl and
  // the NW x split sweep behind DESIGN.md 3.15): one-wave workgroups on 192 (qkv) or 128 x 2 slices (o, down) beat
  // four-wave workgroups on a deeper K split by 15-25 %: fewer slabs, and more workgroups to place per CU
  const int narrowest = rt > (silu ? 2 : 1) ? rt : (silu ? 2 : 1);
  int nw = narrowest;
  while (nw < 4 && row_blocks * gemm_col_groups(n_tiles, nw, silu) > 2 * MI355X_CUS) nw <<= 1;
  const int nw_knob = tune_get(TUNE_LINEAR_NW, 0);
  if (nw_knob == 1 || nw_knob == 2 || nw_knob == 4) nw = nw_knob > narrowest ? nw_knob : narrowest;
  const int64_t col_groups = gemm_col_groups(n_tiles, nw, silu);
  if (col_groups >= ((int64_t)1 << 31)) return SLM_ERR_UNSUPPORTED;

  // K split: the largest that keeps the grid within the CUs and >= 4 chunks per slice; SiLU never splits
  int split = 1;
  if (!silu) {
    const int64_t by_grid = MI355X_CUS / (row_blocks * col_groups);
    split = (int)(by_grid < by_depth ? by_grid : by_depth);
    if (split < 1) split = 1;
    const int sk_knob = tune_get(TUNE_LINEAR_SPLITK, 0);
    if (sk_knob >= 1) {
      const int cap = n_chunks < 1 ? 1 : n_chunks < LIN_MAX_SPLIT ? n_chunks : LIN_MAX_SPLIT;
      split = sk_knob < cap ? sk_knob : cap;
    }
  }
  pl->rt = rt; pl->nw = nw;
  pl->row_blocks = row_blocks; pl->col_groups = col_groups;
  pl->split_k = split; pl->n_chunks = n_chunks; pl->tail_units = (int)((a->K % LIN_KC) / 32);
  // contiguous ranges of whole chunks; the first n_chunks % split slices take one more
  for (int j = 0; j <= LIN_MAX_SPLIT; ++j) pl->slice_chunk[j] = n_chunks;
  const int per = n_chunks / split, extra = n_chunks % split;
  int at = 0;
  for (int j = 0; j < split; ++j) {
    pl->slice_chunk[j] = at;
    at += per + (j < extra ? 1 : 0);
  }
  pl->lds_bytes = (uint64_t)2 * rt * 32 * 256;
  pl->ws_bytes = split > 1 ? (uint64_t)split * a->M * a->N * 4 : 0;
  return SLM_OK;
}

template <typename T, int RT, int NW>
static void launch_linear(const LinearKParams& kp, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((linear_kernel<T, RT, NW>), grid, dim3(NW * 64), 0, st, kp);
}

template <typename T>
static void launch_linear_form(const LinearKParams& kp, int rt, int nw, dim3 grid, hipStream_t st) {
  if (rt == 4) launch_linear<T, 4, 4>(kp, grid, st);
  else if (rt == 2 && nw == 4) launch_linear<T, 2, 4>(kp, grid, st);
  else if (rt == 2) launch_linear<T, 2, 2>(kp, grid, st);
  else if (nw == 4) launch_linear<T, 1, 4>(kp, grid, st);
  else if (nw == 2) launch_linear<T, 1, 2>(kp, grid, st);
  else launch_linear<T, 1, 1>(kp, grid, st);
}

}  // namespace slm

extern "C" {

SLM_API int slm_linear_plan(const slm_linear_args* a, slm_linear_plan_info* out) {
  using namespace slm;
  LinearPlan pl;
  if (!out) return SLM_ERR_INVALID_ARG;
  const int rc = plan_linear(a, &pl);
  if (rc != SLM_OK) return rc;
  *out = slm_linear_plan_info{};
  out->row_tiles = pl.rt; out->waves = pl.nw;
  out->row_blocks = (int32_t)pl.row_blocks; out->col_groups = (int32_t)pl.col_groups;
  out->split_k = pl.split_k; out->n_chunks = pl.n_chunks; out->tail_units = pl.tail_units;
  for (int j = 0; j <= LIN_MAX_SPLIT; ++j) out->slice_chunk[j] = pl.slice_chunk[j];
  out->lds_bytes = pl.lds_bytes; out->workspace_bytes = pl.ws_bytes;
  return SLM_OK;
}

SLM_API size_t slm_linear_workspace_bytes(const slm_linear_args* a) {
  slm::LinearPlan pl;
  return slm::plan_linear(a, &pl) == SLM_OK ? (size_t)pl.ws_bytes : 0;
}

SLM_API int32_t slm_linear_deferred_splits(const slm_linear_args* a) {
  slm::LinearPlan pl;
  return slm::plan_linear(a, &pl) == SLM_OK && (a->flags & SLM_LINEAR_DEFER_REDUCE) && !a->bias && pl.split_k > 1
             ? pl.split_k : 0;
}

SLM_API int slm_linear(const slm_linear_args* a, void* stream) {
  using namespace slm;
  LinearPlan pl;
  const int rc = plan_linear(a, &pl);
  if (rc != SLM_OK) return rc;
  if (a->M == 0) return SLM_OK;
  const bool silu = (a->flags & SLM_LINEAR_SILU_MUL) != 0;
  const bool defer = (a->flags & SLM_LINEAR_DEFER_REDUCE) && !a->bias && pl.split_k > 1;
  if (!a->a || !a->w || !a->c) return SLM_ERR_INVALID_ARG;
  if (a->lda < a->K || a->ldw < a->K || a->ldc < (silu ? a->N / 2 : a->N)) return SLM_ERR_INVALID_ARG;
  if (!aligned16(a->a) || a->lda % 8 || !aligned16(a->w) || a->ldw % 8 || !aligned16(a->c) || a->ldc % 8 ||
      (reinterpret_cast<uintptr_t>(a->bias) & 7u) || !aligned16(a->workspace))
    return SLM_ERR_ALIGNMENT;
  if (pl.ws_bytes > 0 && (!a->workspace || a->workspace_bytes < pl.ws_bytes)) return SLM_ERR_WORKSPACE;

  LinearKParams kp;
  kp.a = reinterpret_cast<const char*>(a->a);
  kp.w = reinterpret_cast<const char*>(a->w);
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
  dispatch_dtype(a->dtype, [&](auto t) { launch_linear_form<decltype(t)>(kp, pl.rt, pl.nw, grid, st); });
  int lrc = hip_check_launch();
  if (lrc != SLM_OK || pl.split_k == 1 || defer) return lrc;
  dispatch_dtype(a->dtype, [&](auto t) {
    launch_splitk_reduce<decltype(t)>(kp.part, a->bias, a->c, a->M, a->N, a->ldc, pl.split_k, st);
  });
  return hip_check_launch();
}

}  // extern "C"
