// dense_fp8.hip -- fp8 (e4m3fn) weight-only linear over checkpoint-layout weights (include/slm_hip.h section 15,
// slm_fp8_linear; the reference's marlin::fp8_gemm, src/kernels/quantization/marlin.h:39-43, which reads a
// Marlin-repacked B -- this kernel reads the checkpoint tensor as it is):
//   C[M, N] = T( (A[M, K] . e4m3(W[N, K])^T) * w_scale[N] + bias[N] ).
//
// dense.hip's kernel with another weight side.  Everything it says about the launch shape holds here: one wave per
// 32-column tile, RT = 1 / 2 / 4 row tiles, NW = 1 / 2 / 4 waves sharing the swizzled [rows][128 k] A image in LDS,
// weights from global memory to registers in 16-B loads with no LDS stage, 128-deep chunks, lane (n = lane & 31,
// h = lane >> 5) owning k = [64 h, 64 h + 64) of the chunk, up to three 32-deep tail units, K slices into fp32
// slabs, and the three epilogues (slab, T(y + bias), SiLU * mul over gate | up wave pairs).  The plan is shared
// (dense_plan.h).
//
// The weight side: a lane's 64 k of a chunk are 64 BYTES of row n, four 16-B loads.  Load j holds k = 64 h + 16 j
// .. + 16, the weight fragments of the two MFMA steps 2 j (dwords 0, 1) and 2 j + 1 (dwords 2, 3); a dword's low
// half is its lower k pair.  e4m3 -> T is exact, two weights per v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0
// (the high half by op_sel): step q of the chunk sees exactly the k -- and the T values -- dense.hip's step q sees
// on T(W), so under the same (RT, NW, split) the accumulators are dense.hip's bit for bit and the A-side LDS
// addressing is unchanged.  A tail unit is one 16-B load per lane half.
//
// w_scale multiplies the fp32 accumulator (never the converter's scale operand): y = acc * w_scale[n], one fp32
// multiply kept out of any contraction with the bias add; a K slice stores y into its slab, so the reduce kernel
// and the deferred consumers see what a dense call leaves.
//
// Ring depth: dense.hip's three chunks, although a chunk of e4m3 is half the bytes in flight.  VMEM completes in
// order, so the wait for the A chunk stored to LDS one iteration ahead leaves F8_RING - 1 weight chunks in flight:
// F8_RING is the depth of BOTH register rings, and the A ring costs 4 P VGPRs a chunk (P = 8 RT / NW 16-B pieces per
// thread) beside the weight ring's 16.  A six-chunk ring was built for the forms with NW >= 2 RT (P <= 4; 264 VGPRs at
// RT 1 x NW 2, one wave per SIMD) and measured on gate_up: 33.8 / 38.4 us at M = 1 / 32 against 29.6 / 35.6 for three
// chunks (profiles/r17_fp8_ring_ab.jsonl), so it is not in the tree.  No result bit depends on F8_RING: a wave's
// MFMAs run in chunk order at any depth.
#include "common.h"
#include "dense_plan.h"
#include "fp8_cvt.h"

namespace slm {

constexpr int F8_RING = 3;   // weight / A register rings (chunks)

struct Fp8LinearKParams {
  const char* a;
  const char* w;
  const float* w_scale;  // [N] or NULL (1.0)
  const void* bias;      // [N] T or NULL
  void* c;
  float* part;           // [split_k][M][N] or NULL (split_k == 1)
  int64_t lda, ldw, ldc;  // elements (ldw: bytes)
  int M, N;
  int n_tiles;       // N / 32
  int tail_units;    // (K % 128) / 32
  int split_k;
  int silu;
  int slice_chunk[LIN_MAX_SPLIT + 1];
};

// (fp8x2_to_t, fp8x8_frag and scaled are fp8_cvt.h's)
template <typename T, int RT, int NW>
__global__ void __launch_bounds__(NW * 64) fp8_linear_kernel(const Fp8LinearKParams p) {
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

  // ---- the slice's chunks ----
  const int c0 = p.slice_chunk[ks];
  const int nC = p.slice_chunk[ks + 1] - c0;
  const int tail_units = ks == p.split_k - 1 ? p.tail_units : 0;
  const uint32_t a_kbase = (uint32_t)c0 * 256u;  // bytes into a row of A
  const uint32_t w_kbase = (uint32_t)c0 * 128u;  // bytes into a row of W

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
    a_src[i] = p.a + 2 * ((int64_t)gr * p.lda + slot * 8) + a_kbase;
    a_dst[i] = stage_swz(row, slot);
  }
  const char* wlane = p.w + ((int64_t)nt * 32 + mrow) * p.ldw + w_kbase;
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
    u32x4 areg[F8_RING][P];
    u32x4 wreg[F8_RING][4];
    auto a_load = [&](int c, u32x4 (&dst)[P]) {
      const uint32_t off = (uint32_t)clampc(c) * 256u;
#pragma unroll
      for (int i = 0; i < P; ++i) dst[i] = *reinterpret_cast<const u32x4*>(a_src[i] + off);
    };
    auto a_store = [&](int stage, const u32x4 (&src)[P]) {
#pragma unroll
      for (int i = 0; i < P; ++i) *reinterpret_cast<u32x4*>(smem + stage * STAGE + a_dst[i]) = src[i];
    };
    // lane half kh: the 64 contiguous bytes [kh * 64, kh * 64 + 64) of the chunk's 128 B of row n
    const char* wl = wlane + kh * 64;
    auto w_load = [&](int c, u32x4 (&w)[4]) {
      const uint32_t off = (uint32_t)clampc(c) * 128u;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = *reinterpret_cast<const u32x4*>(wl + off + j * 16);
    };

    // prologue in the order the steady-state iterations issue (A, then the weights of the same chunk)
    a_load(0, areg[0]);
    w_load(0, wreg[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int d = 1; d < F8_RING; ++d) {
      a_load(d, areg[d]);
      __builtin_amdgcn_sched_barrier(0);
      w_load(d, wreg[d]);
      __builtin_amdgcn_sched_barrier(0);
    }
    a_store(0, areg[0]);
    __syncthreads();

    int stage = 0;
    const int n_iter = (nC + F8_RING - 1) / F8_RING * F8_RING;
    for (int base = 0; base < n_iter; base += F8_RING) {
#pragma unroll
      for (int u = 0; u < F8_RING; ++u) {
        const int i = base + u;  // chunk; ring slot u
        // A for chunk i + F8_RING into the registers chunk i left (stored one iteration ago)
        a_load(i + F8_RING, areg[u]);
        __builtin_amdgcn_sched_barrier(0);
        if (i < nC) {
          const char* sbase = smem + stage * STAGE + a_row;
#pragma unroll
          for (int q = 0; q < 8; ++q) {  // MFMA step q: k = 64 kh + 8 q .. + 8 of the chunk, as in dense.hip
            const u32x4 w16 = wreg[u][q >> 1];
            const frag_t wf = (q & 1) ? fp8x8_frag<T>(w16.z, w16.w) : fp8x8_frag<T>(w16.x, w16.y);
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
        w_load(i + F8_RING, wreg[u]);
        __builtin_amdgcn_sched_barrier(0);
        // chunk i + 1 (loaded F8_RING - 1 iterations ago) -> the buffer everybody finished reading one barrier ago
        a_store(stage ^ 1, areg[(u + 1) % F8_RING]);
        __syncthreads();
        stage ^= 1;
      }
    }
  }

  // ---- K % 128 (last slice): up to three 32-deep units in natural k order, one at a time ----
  if (tail_units > 0) {
    __syncthreads();  // nobody reads the stages any more
#pragma unroll
    for (int i = 0; i < P; ++i) {
      if (a_slot < tail_units * 4)
        *reinterpret_cast<u32x4*>(smem + a_dst[i]) = *reinterpret_cast<const u32x4*>(a_src[i] + (uint32_t)nC * 256u);
    }
    __syncthreads();
    const char* sbase = smem + a_row;
    const char* wt = wlane + (uint32_t)nC * 128u + kh * 16;  // lane half kh: k = 16 kh .. + 16 of a unit
#pragma unroll
    for (int t3 = 0; t3 < 3; ++t3) {
      if (t3 < tail_units) {
        const u32x4 w16 = *reinterpret_cast<const u32x4*>(wt + t3 * 32);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const frag_t wf = s ? fp8x8_frag<T>(w16.z, w16.w) : fp8x8_frag<T>(w16.x, w16.y);
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
  // y = acc * w_scale[n], in place
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 s = {1.f, 1.f, 1.f, 1.f};
    if (p.w_scale) s = *reinterpret_cast<const f32x4*>(p.w_scale + ncol0 + 8 * j);
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      acc[t][4 * j] = scaled(acc[t][4 * j], s.x);
      acc[t][4 * j + 1] = scaled(acc[t][4 * j + 1], s.y);
      acc[t][4 * j + 2] = scaled(acc[t][4 * j + 2], s.z);
      acc[t][4 * j + 3] = scaled(acc[t][4 * j + 3], s.w);
    }
  }
  if (p.part) {  // a K slice: the fp32 slab of scaled sums, no bias, no rounding
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

// ---- host ----
// the section-13 view of the call: slm_fp8_linear_args is slm_linear_args, field for field, plus w_scale
static slm_linear_args as_linear_args(const slm_fp8_linear_args* a) {
  slm_linear_args g;
  g.a = a->a; g.w = a->w; g.bias = a->bias; g.c = a->c;
  g.M = a->M; g.K = a->K; g.N = a->N;
  g.lda = a->lda; g.ldw = a->ldw; g.ldc = a->ldc;
  g.dtype = a->dtype; g.flags = a->flags;
  g.workspace = a->workspace; g.workspace_bytes = a->workspace_bytes;
  return g;
}

static int plan_fp8_linear(const slm_fp8_linear_args* a, LinearPlan* pl) {
  if (!a) return SLM_ERR_INVALID_ARG;
  const slm_linear_args g = as_linear_args(a);
  return plan_linear(&g, pl);
}

template <typename T, int RT, int NW>
static void launch_fp8_linear(const Fp8LinearKParams& kp, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((fp8_linear_kernel<T, RT, NW>), grid, dim3(NW * 64), 0, st, kp);
}

template <typename T>
static void launch_fp8_linear_form(const Fp8LinearKParams& kp, int rt, int nw, dim3 grid, hipStream_t st) {
  if (rt == 4) launch_fp8_linear<T, 4, 4>(kp, grid, st);
  else if (rt == 2 && nw == 4) launch_fp8_linear<T, 2, 4>(kp, grid, st);
  else if (rt == 2) launch_fp8_linear<T, 2, 2>(kp, grid, st);
  else if (nw == 4) launch_fp8_linear<T, 1, 4>(kp, grid, st);
  else if (nw == 2) launch_fp8_linear<T, 1, 2>(kp, grid, st);
  else launch_fp8_linear<T, 1, 1>(kp, grid, st);
}

}  // namespace slm

extern "C" {

SLM_API int slm_fp8_linear_plan(const slm_fp8_linear_args* a, slm_linear_plan_info* out) {
  using namespace slm;
  LinearPlan pl;
  if (!out) return SLM_ERR_INVALID_ARG;
  const int rc = plan_fp8_linear(a, &pl);
  if (rc != SLM_OK) return rc;
  *out = slm_linear_plan_info{};
  out->row_tiles = pl.rt; out->waves = pl.nw;
  out->row_blocks = (int32_t)pl.row_blocks; out->col_groups = (int32_t)pl.col_groups;
  out->split_k = pl.split_k; out->n_chunks = pl.n_chunks; out->tail_units = pl.tail_units;
  for (int j = 0; j <= LIN_MAX_SPLIT; ++j) out->slice_chunk[j] = pl.slice_chunk[j];
  out->lds_bytes = pl.lds_bytes; out->workspace_bytes = pl.ws_bytes;
  return SLM_OK;
}

SLM_API size_t slm_fp8_linear_workspace_bytes(const slm_fp8_linear_args* a) {
  slm::LinearPlan pl;
  return slm::plan_fp8_linear(a, &pl) == SLM_OK ? (size_t)pl.ws_bytes : 0;
}

SLM_API int32_t slm_fp8_linear_deferred_splits(const slm_fp8_linear_args* a) {
  slm::LinearPlan pl;
  return slm::plan_fp8_linear(a, &pl) == SLM_OK && (a->flags & SLM_LINEAR_DEFER_REDUCE) && !a->bias && pl.split_k > 1
             ? pl.split_k : 0;
}

SLM_API int slm_fp8_linear(const slm_fp8_linear_args* a, void* stream) {
  using namespace slm;
  LinearPlan pl;
  const int rc = plan_fp8_linear(a, &pl);
  if (rc != SLM_OK) return rc;
  if (a->M == 0) return SLM_OK;
  const bool silu = (a->flags & SLM_LINEAR_SILU_MUL) != 0;
  const bool defer = (a->flags & SLM_LINEAR_DEFER_REDUCE) && !a->bias && pl.split_k > 1;
  if (!a->a || !a->w || !a->c) return SLM_ERR_INVALID_ARG;
  if (a->lda < a->K || a->ldw < a->K || a->ldc < (silu ? a->N / 2 : a->N)) return SLM_ERR_INVALID_ARG;
  if (!aligned16(a->a) || a->lda % 8 || !aligned16(a->w) || a->ldw % 16 || !aligned16(a->c) || a->ldc % 8 ||
      (reinterpret_cast<uintptr_t>(a->bias) & 7u) || !aligned16(a->w_scale) || !aligned16(a->workspace))
    return SLM_ERR_ALIGNMENT;
  if (pl.ws_bytes > 0 && (!a->workspace || a->workspace_bytes < pl.ws_bytes)) return SLM_ERR_WORKSPACE;

  Fp8LinearKParams kp;
  kp.a = reinterpret_cast<const char*>(a->a);
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
  dispatch_dtype(a->dtype, [&](auto t) { launch_fp8_linear_form<decltype(t)>(kp, pl.rt, pl.nw, grid, st); });
  int lrc = hip_check_launch();
  if (lrc != SLM_OK || pl.split_k == 1 || defer) return lrc;
  dispatch_dtype(a->dtype, [&](auto t) {
    launch_splitk_reduce<decltype(t)>(kp.part, a->bias, a->c, a->M, a->N, a->ldc, pl.split_k, st);
  });
  return hip_check_launch();
}

}  // extern "C"
