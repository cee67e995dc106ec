// w4_moe.hip -- grouped int4-weight x fp16/bf16-activation GEMM over the experts of a mixture-of-experts
// layer (include/slm_hip.h section 10; the role of the reference's Sm80KernelGroupedGemm, src/kernels/gemm/,
// for int4 experts).
//
// For every 32-row block b of the aligned token list (slm_moe_align_block with block_size 32):
//     C[idx, :] = epilogue( A[idx / a_div, :] . dequant(W_e) ),  e = expert_ids[b], idx = sorted[b * 32 + r]
// At decode an expert sees a handful of rows, so the call is a stream of the packed weights of the experts in
// use: the 32-row weight stream of w4_stream32.h (32 x 128 tiles, 4-chunk weight ring, post-scaled dequant
// through the matrix pipe), which w4_small.hip runs over dense rows.  What differs here:
//   * the expert, and with it the base of the weights and of the scale table, is chosen per row tile;
//   * the rows of A are gathered: each thread's two A pointers come from the sorted index list (the issue
//     order and the 32-bit per-chunk offsets are unchanged);
//   * the rows of C are scattered to idx; padding rows (idx == n_flat) load a clamped row and are never stored.
// No split-K (parallelism = blocks x N / 128), hence no workspace.  Workgroups whose block lies beyond the
// device-side n_padded return at once: the grid is sized for the worst case so that a captured graph replays
// for any routing.
#include "w4_stream32.h"
#include "w4_epilogue.h"

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

// NG / SPAN: w4_stream32.h (scale groups per 128-deep chunk; groups wider than a chunk)
template <typename T, int NG, bool SPAN>
__global__ void __launch_bounds__(256, 2) w4a16_moe_gemm_kernel(const MoeGemmKParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_idx[32];  // the block's flat indices, for the scatter in the epilogue
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

  // ---- A: this thread's two (row, 16-B slot) sources of a chunk; the row comes from the sorted list ----
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
    a_dst[i] = stage_swz(row, slot);
  }

  // the expert base is a 64-bit pointer, offsets inside an expert 32-bit
  const char* wlane = p.wq + (int64_t)e * p.wq_stride + (nt * 64 + lane) * 16;
  const char* szlane = p.sz + (int64_t)e * p.sz_stride + (nt * 32 + (lane & 31)) * 4;
  const uint32_t wstride = (uint32_t)(n_tiles * 1024);  // bytes per 64-deep half chunk
  const uint32_t szstride = (uint32_t)(p.N * 4);        // bytes per scale group
  const f32x16 acc[1] = {w4_stream32<T, NG, SPAN>(smem, a_src, a_dst, wlane, szlane, wstride, szstride,
                                                  w4_cpg_shift(p.gs_shift), 0, p.n_chunks, lane & 31, lane >> 5)};

  // ---- epilogue (C/D layout: w4_epilogue.h); the row goes to C[idx]; s_idx was written before the first barrier
  const ScatterRows rows{s_idx, p.n_flat, p.row_scale};
  if (p.silu) {
    // SLM_W4_SILU_MUL: waves (0, 1) and (2, 3) hold a (gate, up) tile pair
    uint16_t* ex = reinterpret_cast<uint16_t*>(smem) + (wave >> 1) * 1024;
    cd_silu_exchange<T, 1>(acc, rows, lane, ex, wave & 1, !(wave & 1) && nvalid, nullptr, 0, p.c, p.ldc, nt >> 1);
    return;
  }
  if (!nvalid) return;
  cd_store<T, 1>(acc, rows, lane, p.c, p.ldc, nt, 0.f);
}

template <typename T, int NG, bool SPAN>
static void launch_moe_t(const MoeGemmKParams& kp, unsigned n_blocks, hipStream_t st) {
  hipLaunchKernelGGL((w4a16_moe_gemm_kernel<T, NG, SPAN>), dim3(n_blocks), dim3(256),
                     S32_LDS_BYTES, st, kp);
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
  if (!w4_format_bits_ok(a->format)) return SLM_ERR_INVALID_ARG;
  if (!w4_format_valid(a->format)) return SLM_ERR_UNSUPPORTED;  // 8-bit planes need the column gather
  if (a->perm || a->bias) return SLM_ERR_UNSUPPORTED;
  if (a->K % W4_KC || a->N % 64) return SLM_ERR_UNSUPPORTED;
  if (a->flags & ~SLM_W4_SILU_MUL) return SLM_ERR_INVALID_ARG;
  const bool silu = (a->flags & SLM_W4_SILU_MUL) != 0;
  if (silu && (!(a->format & SLM_W4_PAIRED) || a->row_scale)) return SLM_ERR_INVALID_ARG;
  const int64_t gs = a->group_size;
  if (!w4_group_size_valid(gs, a->K)) return SLM_ERR_UNSUPPORTED;
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
  dispatch_dtype(a->dtype, [&](auto t) { launch_moe_ng<decltype(t)>(kp, ng, (unsigned)grid, st); });
  return hip_check_launch();
}

}  // extern "C"
