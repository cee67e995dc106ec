// w4_moe.hip -- grouped int4-weight x fp16/bf16-activation GEMM over the experts of a mixture-of-experts
// layer (include/slm_hip.h section 10; the role of the reference's Sm80KernelGroupedGemm, src/kernels/gemm/,
// for int4 experts).
//
// For every 32-row block b of the aligned token list (slm_moe_align_block with block_size 32):
//     C[idx, :] = epilogue( A[idx / a_div, :] . dequant(W_e) ),  e = expert_ids[b], idx = sorted[b * 32 + r]
// At decode an expert sees a handful of rows, so the call is a stream of the packed weights of the experts in
// use: this is w4_small.hip's kernel -- 32 x 128 tiles, 4-chunk weight ring, post-scaled dequant through the
// matrix pipe, SiLU*mul epilogue; read its header and comments for why the loads are issued in this order and
// pinned with sched_barriers -- with three changes:
//   * the expert, and with it the base of the weights and of the scale table, is chosen per row tile;
//   * the rows of A are gathered: each thread's two A pointers come from the sorted index list (the issue
//     order and the 32-bit per-chunk offsets are unchanged);
//   * the rows of C are scattered to idx; padding rows (idx == n_flat) load a clamped row and are never stored.
// No split-K (parallelism = blocks x N / 128), hence no workspace.  Workgroups whose block lies beyond the
// device-side n_padded return at once: the grid is sized for the worst case so that a captured graph replays
// for any routing.
#include "w4_common.h"

namespace slm {

struct MoeGemmKParams {
  const void* a;
  const char* wq;           // expert 0
  const char* sz;
  void* c;
  const float* row_scale;   // [n_flat] or NULL
  const int32_t* sorted;    // [>= n_padded]
  const int32_t* expert_ids;
  const int32_t* n_padded;  // [1]
  int64_t wq_stride, sz_stride;  // bytes per expert
  int64_t N, lda, ldc;
  int n_flat;               // rows of c; indices >= n_flat are padding
  int a_div;
  int n_experts;
  int gs_shift;
  int n_chunks;             // K / 128
  int n_nblocks;
  int silu;
};

constexpr int MOE_STAGES = 2;
constexpr int MOE_STAGE_BYTES = 32 * 256;
constexpr int MOE_RING = 4;

template <typename T>
struct MoeOnes;
template <>
struct MoeOnes<bf16_tag> {
  static constexpr uint32_t bits = 0x3F803F80u;
};
template <>
struct MoeOnes<f16_tag> {
  static constexpr uint32_t bits = 0x3C003C00u;
};

// NG / SPAN: as in w4_small.hip (scale groups per 128-deep chunk; groups wider than a chunk)
template <typename T, int NG, bool SPAN>
__global__ void __launch_bounds__(256, 2) w4a16_moe_gemm_kernel(const MoeGemmKParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_idx[32];  // the block's flat indices, for the scatter in the epilogue
  typedef typename Mfma<T>::frag frag_t;
  constexpr int WPG = 8 / NG;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nb = blockIdx.x % p.n_nblocks;
  const int mb = blockIdx.x / p.n_nblocks;
  if ((int64_t)mb * 32 >= (int64_t)p.n_padded[0]) return;  // beyond the aligned list: nothing to do
  const int e = p.expert_ids[mb];
  if ((unsigned)e >= (unsigned)p.n_experts) return;        // never produced by the align step
  const int64_t n_tiles = p.N / 32;
  int64_t nt = (int64_t)nb * 4 + wave;
  const bool nvalid = nt < n_tiles;
  if (!nvalid) nt = n_tiles - 1;  // clamped duplicate work, never stored

  const int nC = p.n_chunks;  // >= 1
  const int last = nC - 1;
  auto clampc = [&](int c) { return c < last ? c : last; };

  // ---- A staging: thread -> (row, 16-B slot) x 2 per chunk; the row comes from the sorted list ----
  const int32_t* blk = p.sorted + (int64_t)mb * 32;
  if (tid < 32) s_idx[tid] = blk[tid];
  const char* abase = reinterpret_cast<const char*>(p.a);
  const char* a_src[2];
  int a_dst[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int idx = tid + 256 * i;
    const int row = idx >> 4, slot = idx & 15;
    const int fi = blk[row];
    const int64_t ar = (unsigned)fi < (unsigned)p.n_flat ? fi / p.a_div : 0;  // padding: a clamped row
    a_src[i] = abase + 2 * (ar * p.lda + slot * 8);
    a_dst[i] = row * 256 + ((slot ^ (row & 15)) << 4);
  }
  u32x4 areg[MOE_RING][2];
  auto a_load = [&](int c, u32x4 (&dst)[2]) {
    const uint32_t off = (uint32_t)clampc(c) * 256u;
#pragma unroll
    for (int i = 0; i < 2; ++i) dst[i] = *reinterpret_cast<const u32x4*>(a_src[i] + off);
  };
  auto a_store = [&](int stage, const u32x4 (&src)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      *reinterpret_cast<u32x4*>(smem + stage * MOE_STAGE_BYTES + a_dst[i]) = src[i];
  };

  // ---- weight / scale rings: the expert base is a 64-bit pointer, offsets inside an expert 32-bit ----
  u32x4 wreg[MOE_RING][2];
  uint32_t szreg[MOE_RING][NG];
  const char* wlane = p.wq + (int64_t)e * p.wq_stride + (nt * 64 + lane) * 16;
  const char* szlane = p.sz + (int64_t)e * p.sz_stride + (nt * 32 + (lane & 31)) * 4;
  const uint32_t wstride = (uint32_t)(n_tiles * 1024);  // bytes per 64-deep half chunk
  const uint32_t szstride = (uint32_t)(p.N * 4);        // bytes per scale group
  const int cpg_shift = p.gs_shift >= 30 ? 30 : (p.gs_shift > 7 ? p.gs_shift - 7 : 0);
  auto w_load = [&](int c, u32x4 (&w)[2], uint32_t (&sz)[NG]) {
    const uint32_t cc = (uint32_t)clampc(c);
#pragma unroll
    for (int h = 0; h < 2; ++h)
      w[h] = __builtin_nontemporal_load(
          reinterpret_cast<const u32x4*>(wlane + (cc * 2 + h) * wstride));
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const uint32_t grp = NG > 1 ? cc * NG + g : (cc >> cpg_shift);
      sz[g] = *reinterpret_cast<const uint32_t*>(szlane + grp * szstride);
    }
  };

  // prologue in the order the steady-state iterations issue (w4_small.hip)
  a_load(0, areg[0]);
  w_load(0, wreg[0], szreg[0]);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int d = 1; d < MOE_RING; ++d) {
    a_load(d, areg[d]);
    __builtin_amdgcn_sched_barrier(0);
    w_load(d, wreg[d], szreg[d]);
    __builtin_amdgcn_sched_barrier(0);
  }
  a_store(0, areg[0]);

  f32x16 acc, tmp, tmpx;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = tmp[r] = tmpx[r] = 0.f;
  const u32x4 ones4 = {MoeOnes<T>::bits, MoeOnes<T>::bits, MoeOnes<T>::bits, MoeOnes<T>::bits};
  const frag_t ones = __builtin_bit_cast(frag_t, ones4);
  uint32_t magic_v = W4Magic<T>::bits;
  asm volatile("" : "+v"(magic_v));
  uint32_t mask_s = 0x000F000Fu;
  asm volatile("" : "+s"(mask_s));
  const int mrow = lane & 31, kh = lane >> 5;
  const int a_row = mrow * 256;
  const int a_swz = mrow & 15;

  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

  bool group_open = false;
  int stage = 0;
  const int n_iter = (nC + MOE_RING - 1) / MOE_RING * MOE_RING;
  for (int base = 0; base < n_iter; base += MOE_RING) {
#pragma unroll
    for (int u = 0; u < MOE_RING; ++u) {
      const int i = base + u;
      a_load(i + MOE_RING, areg[u]);
      __builtin_amdgcn_sched_barrier(0);
      if (i < nC) {
        const char* sbase = smem + stage * MOE_STAGE_BYTES + a_row;
        const bool grp_ends = !SPAN || i == nC - 1 || ((i + 1) >> cpg_shift) != (i >> cpg_shift);
        frag_t af = __builtin_bit_cast(
            frag_t, *reinterpret_cast<const u32x4*>(sbase + (((0 * 2 + kh) ^ a_swz) << 4)));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          frag_t af_n = af;
          if (j < 7)
            af_n = __builtin_bit_cast(
                frag_t, *reinterpret_cast<const u32x4*>(sbase + ((((j + 1) * 2 + kh) ^ a_swz) << 4)));
          const u32x4 wv = wreg[u][j >> 2];
          const uint32_t word = (j & 3) == 0 ? wv.x : (j & 3) == 1 ? wv.y : (j & 3) == 2 ? wv.z : wv.w;
          uint32_t o[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            // a plain expression, not inline asm (w4_small.hip: hazards behind an asm statement)
            const uint32_t x = q == 0 ? word : word >> (4 * q);
            o[q] = (x & mask_s) | magic_v;
          }
          const u32x4 packed = {o[0], o[1], o[2], o[3]};
          const frag_t bf = __builtin_bit_cast(frag_t, packed);
          const bool g_first = (j % WPG) == 0 && !(SPAN && group_open);
          if (g_first) {
            f32x16 z;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = 0.f;
            tmp = Mfma<T>::run(af, bf, z);
            tmpx = Mfma<T>::run(af, ones, z);
          } else {
            tmp = Mfma<T>::run(af, bf, tmp);
            tmpx = Mfma<T>::run(af, ones, tmpx);
          }
          const bool g_last = (j % WPG) == WPG - 1;
          if (g_last && (!SPAN || grp_ends)) {
            float sc, zm;
            W4Magic<T>::decode(szreg[u][j / WPG], sc, zm);
            const float nzs = -zm * sc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = fmaf(sc, tmp[r], fmaf(nzs, tmpx[r], acc[r]));
          }
          af = af_n;
        }
        if constexpr (SPAN) group_open = !grp_ends;
      }
      __builtin_amdgcn_sched_barrier(0);
      w_load(i + MOE_RING, wreg[u], szreg[u]);
      __builtin_amdgcn_sched_barrier(0);
      a_store(stage ^ 1, areg[(u + 1) % MOE_RING]);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      stage ^= 1;
    }
  }

  // ---- epilogue: C/D layout of the 32x32 MFMA: col = lane & 31, row = (r&3) + 8*(r>>2) + 4*(lane>>5);
  // the row goes to C[idx]; s_idx was written before the first barrier
  const int64_t ncol = nt * 32 + (lane & 31);
  uint16_t* cbase = reinterpret_cast<uint16_t*>(p.c);
  if (p.silu) {
    // SLM_W4_SILU_MUL: waves (0, 1) and (2, 3) hold a (gate, up) tile pair; the up wave hands its
    // T-rounded tile to the gate wave through the (now idle) A buffers; same lane, same r
    uint16_t* ex = reinterpret_cast<uint16_t*>(smem) + (wave >> 1) * 1024;
    if (wave & 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) ex[r * 64 + lane] = pack1<T>(acc[r]);
    }
    __syncthreads();
    if ((wave & 1) || !nvalid) return;
    const int64_t ocol = (nt >> 1) * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int fi = s_idx[(r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)];
      const float g = lo_f32<T>((uint32_t)pack1<T>(acc[r]));
      const float u = lo_f32<T>((uint32_t)ex[r * 64 + lane]);
      if ((unsigned)fi < (unsigned)p.n_flat) cbase[(int64_t)fi * p.ldc + ocol] = pack1<T>(silu_mul1(g, u));
    }
    return;
  }
  if (!nvalid) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int fi = s_idx[(r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)];
    if ((unsigned)fi < (unsigned)p.n_flat) {
      float v = acc[r];
      if (p.row_scale) v *= p.row_scale[fi];
      cbase[(int64_t)fi * p.ldc + ncol] = pack1<T>(v);
    }
  }
}

template <typename T, int NG, bool SPAN>
static void launch_moe_t(const MoeGemmKParams& kp, unsigned n_blocks, hipStream_t st) {
  hipLaunchKernelGGL((w4a16_moe_gemm_kernel<T, NG, SPAN>), dim3(n_blocks), dim3(256),
                     MOE_STAGES * MOE_STAGE_BYTES, st, kp);
}

template <typename T>
static void launch_moe_ng(const MoeGemmKParams& kp, int ng, unsigned n_blocks, hipStream_t st) {
  if (ng == 4) launch_moe_t<T, 4, false>(kp, n_blocks, st);
  else if (ng == 2) launch_moe_t<T, 2, false>(kp, n_blocks, st);
  else if (kp.gs_shift == 7) launch_moe_t<T, 1, false>(kp, n_blocks, st);  // group 128
  else launch_moe_t<T, 1, true>(kp, n_blocks, st);
}

}  // namespace slm

extern "C" {

SLM_API int slm_moe_w4a16_gemm(const slm_moe_gemm_args* a, void* stream) {
  using namespace slm;
  if (!a) return SLM_ERR_INVALID_ARG;
  if (a->n_flat < 0 || a->K <= 0 || a->N <= 0 || a->a_div < 1 || a->n_experts < 1 || a->max_blocks < 0)
    return SLM_ERR_INVALID_ARG;
  if (a->dtype != SLM_F16 && a->dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  const int base = a->format & SLM_W4_FORMAT_MASK;
  if (a->format & ~(SLM_W4_FORMAT_MASK | SLM_W4_PAIRED)) return SLM_ERR_INVALID_ARG;
  if (base != SLM_W4_GPTQ && base != SLM_W4_AWQ) return SLM_ERR_UNSUPPORTED;  // 8-bit planes need the column gather
  if (a->perm || a->bias) return SLM_ERR_UNSUPPORTED;
  if (a->K % W4_KC || a->N % 64) return SLM_ERR_UNSUPPORTED;
  if (a->flags & ~SLM_W4_SILU_MUL) return SLM_ERR_INVALID_ARG;
  const bool silu = (a->flags & SLM_W4_SILU_MUL) != 0;
  if (silu && (!(a->format & SLM_W4_PAIRED) || a->row_scale)) return SLM_ERR_INVALID_ARG;
  const int64_t gs = a->group_size;
  if (!(gs == 32 || gs == 64 || (gs >= 128 && is_pow2(gs)) || gs == a->K)) return SLM_ERR_UNSUPPORTED;
  if (a->K % gs) return SLM_ERR_UNSUPPORTED;
  // 32-bit offsets inside one expert (w4_small.hip's rules, per expert); flat indices are int32
  if (a->K * a->N / 2 >= ((int64_t)1 << 32) || (a->K / gs) * a->N * 4 >= ((int64_t)1 << 32) ||
      a->n_flat >= ((int64_t)1 << 31) - 256)
    return SLM_ERR_UNSUPPORTED;
  if (a->n_flat == 0 || a->max_blocks == 0) return SLM_OK;
  if (!a->a || !a->wq || !a->sz || !a->c || !a->sorted_token_idxes || !a->expert_ids || !a->n_padded_tokens)
    return SLM_ERR_INVALID_ARG;
  if (a->wq_expert_stride < a->K * a->N / 2 || a->sz_expert_stride < (a->K / gs) * a->N * 4) return SLM_ERR_INVALID_ARG;
  if (!aligned16(a->a) || a->lda % 8 || a->lda < a->K || !aligned16(a->wq) || a->wq_expert_stride % 16 ||
      (reinterpret_cast<uintptr_t>(a->sz) & 3u) || a->sz_expert_stride % 4 || a->ldc < (silu ? a->N / 2 : a->N))
    return SLM_ERR_ALIGNMENT;
  const int64_t n_nblocks = (a->N / 32 + 3) / 4;
  const int64_t grid = (int64_t)a->max_blocks * n_nblocks;
  if (grid >= ((int64_t)1 << 31)) return SLM_ERR_UNSUPPORTED;

  MoeGemmKParams kp;
  kp.a = a->a;
  kp.wq = reinterpret_cast<const char*>(a->wq);
  kp.sz = reinterpret_cast<const char*>(a->sz);
  kp.c = a->c;
  kp.row_scale = a->row_scale;
  kp.sorted = a->sorted_token_idxes;
  kp.expert_ids = a->expert_ids;
  kp.n_padded = a->n_padded_tokens;
  kp.wq_stride = a->wq_expert_stride; kp.sz_stride = a->sz_expert_stride;
  kp.N = a->N; kp.lda = a->lda; kp.ldc = a->ldc;
  kp.n_flat = (int)a->n_flat;
  kp.a_div = a->a_div;
  kp.n_experts = a->n_experts;
  kp.gs_shift = gs == a->K ? 30 : ilog2(gs);  // per-channel: every k maps to group 0
  kp.n_chunks = (int)(a->K / W4_KC);
  kp.n_nblocks = (int)n_nblocks;
  kp.silu = silu ? 1 : 0;
  const int ng = gs == 32 ? 4 : gs == 64 ? 2 : 1;
  hip_clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (a->dtype == SLM_BF16) launch_moe_ng<bf16_tag>(kp, ng, (unsigned)grid, st);
  else launch_moe_ng<f16_tag>(kp, ng, (unsigned)grid, st);
  return hip_check_launch();
}

}  // extern "C"
