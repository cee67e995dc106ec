// moe_gemm_fp8.hip -- grouped fp8 (e4m3fn) weight-only GEMM over the experts of a mixture-of-experts layer
// (include/slm_hip.h section 16, slm_moe_fp8_gemm).
//
// For every 32-row block b of the aligned token list (slm_moe_align_block with block_size 32):
//     C[idx, :] = epilogue( (A[idx / a_div, :] . e4m3(W_e)^T) * w_scale[e, :] ),  e = expert_ids[b], idx = sorted[b * 32 + r]
// moe_gemm.hip's kernel with dense_fp8.hip's weight side.  Everything moe_gemm.hip says about the aligned list, the
// decomposition (one wave per 32 x 32 tile over the whole K, NW = 4 / 2 / 1 waves sharing the swizzled [32][128 k]
// A image, moe_gemm_waves), the A pipeline and the SiLU * mul wave pairs holds here.
//
// The weight side: W_e is the checkpoint tensor [N, K] in bytes.  A lane's 64 k of a 128-deep chunk are 64
// contiguous BYTES of row n, four 16-B loads; lane half h takes bytes [64 h, 64 h + 64) of the chunk's 128 B.  Load j
// holds k = 64 h + 16 j .. + 16, the weight fragments of the two MFMA steps 2 j (dwords 0, 1) and 2 j + 1 (dwords
// 2, 3).  e4m3 -> T is exact, two weights per v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0 (fp8_cvt.h): step q of
// a chunk sees exactly the k -- and the T values -- moe_gemm.hip's step q sees on T(W), so the accumulators are
// moe_gemm.hip's bit for bit and the A-side LDS addressing is unchanged.  A tail unit (32 k) is one 16-B load per
// lane half.
//
// Scale.  In the C layout of the 32x32 MFMA a lane holds ONE column (col = lane & 31): one scale load per lane,
// w_scale[e * scale_stride + n].  It multiplies the fp32 accumulator (never the converter's scale operand), then
// row_scale[idx] multiplies that product, then one rounding.  Under SiLU * mul the gate and the up wave each scale
// their tile by their own channels before the T rounding and the LDS hand-over.
//
// Ring depth: three chunks for both rings, as dense_fp8.hip found (its header: a six-chunk ring measured slower).
// No result bit depends on it.
#include "common.h"
#include "fp8_cvt.h"
#include "moe_gemm_plan.h"

namespace slm {

struct MoeFp8KParams {
  const void* a;
  const char* w;            // expert 0
  const float* w_scale;     // expert 0's [N], or NULL (1.0)
  void* c;
  const float* row_scale;   // [n_flat] or NULL
  const int32_t* sorted;    // [>= n_padded]
  const int32_t* expert_ids;
  const int32_t* n_padded;  // [1]
  int64_t w_stride;         // bytes per expert
  int64_t scale_stride;     // floats per expert
  int64_t lda, ldw, ldc;    // elements (ldw: bytes)
  int n_flat;               // rows of c; indices >= n_flat are padding
  int a_div;
  int n_experts;
  int n_tiles;              // N / 32
  int n_chunks;             // K / 128
  int tail_units;           // (K % 128) / 32
  int n_nblocks;            // workgroups per row block
  int silu;
};

template <typename T, int NW>
__global__ void __launch_bounds__(NW * 64) moe_fp8_gemm_kernel(const MoeFp8KParams p) {
  typedef typename Mfma<T>::frag frag_t;
  constexpr int NT = NW * 64;
  constexpr int P = 512 / NT;  // 16-B pieces of a chunk of A per thread
  __shared__ __attribute__((aligned(16))) char smem[MG_LDS_BYTES];
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

  // ---- A: this thread's P (row, 16-B slot) sources of a chunk; the row comes from the sorted list ----
  const int32_t* blk = p.sorted + (int64_t)mb * 32;
  if (tid < 32) s_idx[tid] = blk[tid];
  const char* abase = reinterpret_cast<const char*>(p.a);
  const char* a_src[P];
  int a_dst[P];
  const int a_slot = tid & 15;  // NT % 16 == 0: one slot for all of a thread's pieces
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int idx = tid + NT * i;
    const int row = idx >> 4, slot = idx & 15;
    const int fi = blk[row];
    const int64_t ar = (unsigned)fi < (unsigned)p.n_flat ? fi / p.a_div : 0;  // padding: a clamped row
    a_src[i] = abase + 2 * (ar * p.lda + slot * 8);
    a_dst[i] = stage_swz(row, slot);
  }
  // the expert base is a 64-bit pointer, offsets inside an expert 32-bit
  const int ncol = nt * 32 + mrow;  // the lane's row of W_e = its column of C (clamped tiles: a valid duplicate)
  const char* wlane = p.w + (int64_t)e * p.w_stride + (int64_t)ncol * p.ldw;
  const int a_row = mrow * 256;
  const int a_swz = mrow & 15;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  const int nC = p.n_chunks;
  if (nC > 0) {
    const int last = nC - 1;
    auto clampc = [&](int c) { return c < last ? c : last; };
    u32x4 areg[MG_RING][P];
    u32x4 wreg[MG_RING][4];
    auto a_load = [&](int c, u32x4 (&dst)[P]) {
      const uint32_t off = (uint32_t)clampc(c) * 256u;
#pragma unroll
      for (int i = 0; i < P; ++i) dst[i] = *reinterpret_cast<const u32x4*>(a_src[i] + off);
    };
    auto a_store = [&](int stage, const u32x4 (&src)[P]) {
#pragma unroll
      for (int i = 0; i < P; ++i) *reinterpret_cast<u32x4*>(smem + stage * MG_STAGE_BYTES + a_dst[i]) = src[i];
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
    for (int d = 1; d < MG_RING; ++d) {
      a_load(d, areg[d]);
      __builtin_amdgcn_sched_barrier(0);
      w_load(d, wreg[d]);
      __builtin_amdgcn_sched_barrier(0);
    }
    a_store(0, areg[0]);
    __syncthreads();

    int stage = 0;
    const int n_iter = (nC + MG_RING - 1) / MG_RING * MG_RING;
    for (int base = 0; base < n_iter; base += MG_RING) {
#pragma unroll
      for (int u = 0; u < MG_RING; ++u) {
        const int i = base + u;  // chunk; ring slot u
        // A for chunk i + 3 into the registers chunk i left (stored one iteration ago)
        a_load(i + MG_RING, areg[u]);
        __builtin_amdgcn_sched_barrier(0);
        if (i < nC) {
          const char* sbase = smem + stage * MG_STAGE_BYTES + a_row;
#pragma unroll
          for (int q = 0; q < 8; ++q) {  // MFMA step q: k = 64 kh + 8 q .. + 8 of the chunk, as in moe_gemm.hip
            const u32x4 w16 = wreg[u][q >> 1];
            const frag_t wf = (q & 1) ? fp8x8_frag<T>(w16.z, w16.w) : fp8x8_frag<T>(w16.x, w16.y);
            const frag_t af = __builtin_bit_cast(
                frag_t, *reinterpret_cast<const u32x4*>(sbase + (((kh * 8 + q) ^ a_swz) << 4)));
            acc = Mfma<T>::run(af, wf, acc);
          }
        }
        // the refill AFTER the old values are consumed (pinned): each ring slot keeps its registers
        __builtin_amdgcn_sched_barrier(0);
        w_load(i + MG_RING, wreg[u]);
        __builtin_amdgcn_sched_barrier(0);
        // chunk i + 1 (loaded two iterations ago) -> the buffer everybody finished reading one barrier ago
        a_store(stage ^ 1, areg[(u + 1) % MG_RING]);
        __syncthreads();
        stage ^= 1;
      }
    }
  }

  // ---- K % 128: up to three 32-deep units in natural k order, one at a time ----
  if (p.tail_units > 0) {
    __syncthreads();  // nC == 0: s_idx; otherwise nobody reads the stages any more
#pragma unroll
    for (int i = 0; i < P; ++i) {
      if (a_slot < p.tail_units * 4)
        *reinterpret_cast<u32x4*>(smem + a_dst[i]) = *reinterpret_cast<const u32x4*>(a_src[i] + (uint32_t)nC * 256u);
    }
    __syncthreads();
    const char* sbase = smem + a_row;
    const char* wt = wlane + (uint32_t)nC * 128u + kh * 16;  // lane half kh: k = 16 kh .. + 16 of a unit
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      if (t < p.tail_units) {
        const u32x4 w16 = *reinterpret_cast<const u32x4*>(wt + t * 32);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const frag_t wf = s ? fp8x8_frag<T>(w16.z, w16.w) : fp8x8_frag<T>(w16.x, w16.y);
          const frag_t af = __builtin_bit_cast(
              frag_t, *reinterpret_cast<const u32x4*>(sbase + (((t * 4 + kh * 2 + s) ^ a_swz) << 4)));
          acc = Mfma<T>::run(af, wf, acc);
        }
      }
    }
    __syncthreads();  // the SiLU exchange below reuses the stage
  }

  // ---- y = acc * w_scale[e, n]: the lane's one column, one fp32 multiply per element, in place ----
  if (p.w_scale) {
    const float s = p.w_scale[(int64_t)e * p.scale_stride + ncol];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = scaled(acc[r], s);
  }

  // ---- epilogue (moe_gemm.hip): col = lane & 31, row = (r&3) + 8*(r>>2) + 4*(lane>>5); the row goes to C[idx] ----
  uint16_t* cbase = reinterpret_cast<uint16_t*>(p.c);
  if constexpr (NW >= 2) {
    if (p.silu) {
      // the up wave hands its T-rounded tile to the gate wave through the (now idle) A buffers; same lane, same r
      uint16_t* ex = reinterpret_cast<uint16_t*>(smem) + (wave >> 1) * 1024;
      if (wave & 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) ex[r * 64 + lane] = pack1<T>(acc[r]);
      }
      __syncthreads();
      if ((wave & 1) || !nvalid) return;
#pragma unroll
      for (int r = 0; r < 16; ++r) {  // the gate wave: nt = the output tile, ncol the output column
        const int fi = s_idx[(r & 3) + 8 * (r >> 2) + 4 * kh];
        const float g = lo_f32<T>((uint32_t)pack1<T>(acc[r]));
        const float u = lo_f32<T>((uint32_t)ex[r * 64 + lane]);
        if ((unsigned)fi < (unsigned)p.n_flat) cbase[(int64_t)fi * p.ldc + ncol] = pack1<T>(silu_mul1(g, u));
      }
      return;
    }
  }
  if (!nvalid) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int fi = s_idx[(r & 3) + 8 * (r >> 2) + 4 * kh];
    if ((unsigned)fi < (unsigned)p.n_flat) {
      float v = acc[r];
      if (p.row_scale) v *= p.row_scale[fi];
      cbase[(int64_t)fi * p.ldc + ncol] = pack1<T>(v);
    }
  }
}

template <typename T, int NW>
static void launch_moe_fp8(const MoeFp8KParams& kp, unsigned grid, hipStream_t st) {
  hipLaunchKernelGGL((moe_fp8_gemm_kernel<T, NW>), dim3(grid), dim3(NW * 64), 0, st, kp);
}

template <typename T>
static void launch_moe_fp8_nw(const MoeFp8KParams& kp, int nw, unsigned grid, hipStream_t st) {
  if (nw == 4) launch_moe_fp8<T, 4>(kp, grid, st);
  else if (nw == 2) launch_moe_fp8<T, 2>(kp, grid, st);
  else launch_moe_fp8<T, 1>(kp, grid, st);
}

}  // namespace slm

extern "C" {

SLM_API int slm_moe_fp8_gemm(const slm_moe_fp8_gemm_args* a, void* stream) {
  using namespace slm;
  if (!a) return SLM_ERR_INVALID_ARG;
  if (a->n_flat < 0 || a->K <= 0 || a->N <= 0 || a->a_div < 1 || a->n_experts < 1 || a->max_blocks < 0)
    return SLM_ERR_INVALID_ARG;
  if (a->dtype != SLM_F16 && a->dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (a->flags & ~SLM_MOE_SILU_MUL) return SLM_ERR_INVALID_ARG;
  const bool silu = (a->flags & SLM_MOE_SILU_MUL) != 0;
  if (silu && a->row_scale) return SLM_ERR_INVALID_ARG;
  if (a->K % 32 || a->N % 32 || (silu && (a->N / 2) % 32)) return SLM_ERR_UNSUPPORTED;
  // 32-bit offsets inside one expert (N >= 32: inside a row of A too); flat indices are int32
  if (a->K * a->N >= ((int64_t)1 << 32) || a->n_flat >= ((int64_t)1 << 31) - 256) return SLM_ERR_UNSUPPORTED;
  if (a->n_flat == 0 || a->max_blocks == 0) return SLM_OK;
  if (!a->a || !a->w || !a->c || !a->sorted_token_idxes || !a->expert_ids || !a->n_padded_tokens)
    return SLM_ERR_INVALID_ARG;
  const int64_t n_out = silu ? a->N / 2 : a->N;
  if (a->lda < a->K || a->ldw < a->K || a->ldc < n_out || a->w_expert_stride < (a->N - 1) * a->ldw + a->K)
    return SLM_ERR_INVALID_ARG;
  if (a->w_scale && a->w_scale_expert_stride < a->N) return SLM_ERR_INVALID_ARG;
  if (!aligned16(a->a) || a->lda % 8 || !aligned16(a->w) || a->ldw % 16 || a->w_expert_stride % 16 ||
      (reinterpret_cast<uintptr_t>(a->c) & 1u) || (reinterpret_cast<uintptr_t>(a->row_scale) & 3u) ||
      (reinterpret_cast<uintptr_t>(a->w_scale) & 3u))
    return SLM_ERR_ALIGNMENT;
  if (a->N * a->ldw >= ((int64_t)1 << 32)) return SLM_ERR_UNSUPPORTED;  // a strided expert: still < 4 GiB
  const int64_t n_tiles = a->N / 32;
  const int nw = moe_gemm_waves(a->max_blocks, n_tiles, silu);
  const int64_t n_nblocks = gemm_col_groups(n_tiles, nw, silu);
  const int64_t grid = (int64_t)a->max_blocks * n_nblocks;
  if (grid >= ((int64_t)1 << 31)) return SLM_ERR_UNSUPPORTED;

  MoeFp8KParams kp;
  kp.a = a->a;
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
  dispatch_dtype(a->dtype, [&](auto t) { launch_moe_fp8_nw<decltype(t)>(kp, nw, (unsigned)grid, st); });
  return hip_check_launch();
}

}  // extern "C"
