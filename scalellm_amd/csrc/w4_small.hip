// w4_small.hip -- int4-weight x fp16/bf16-activation GEMM for M <= 32 (decode at small batch):
// a lean weight-streaming kernel.
//
// Same operator as w4.hip (replaces marlin::gptq_gemm, reference gptq_gemm.cu:585-710, on the
// small-batch decode shapes), same packed layout and scale/zero table (w4.hip header).
//
// At M <= 32 the GEMM is a pure HBM stream of the packed weights (58.7 MB for the Llama-3-8B
// gate_up layer = 8.4 us at 7 TB/s) and the cost that matters is INSTRUCTIONS PER WEIGHT WORD: a
// gfx950 SIMD issues about one instruction per 4 cycles in total, and the general kernel's small-M
// instantiation spent ~35 instructions per 8-weight word (measured, SQ_INSTS_*: 24 VALU + 7 SALU +
// LDS/waits), which alone is 16 us on this layer whatever the occupancy or split-K.  This kernel
// spends ~15:
//   * post-scaled form: the MFMA consumes the raw magic-number values (magic + q, exact in T);
//     unpack = shift + and_or per nibble pair.  The affine part is applied per scale group:
//         sum_k x_k s (q_k - z) = s * ( T - (magic + z) * X ),  T = sum_k x_k (magic + q_k),
//     X = sum_k x_k.  X comes out of the matrix pipe as well -- a second MFMA per k-step against a
//     constant all-ones B fragment, in exactly the accumulator layout the epilogue needs -- so no
//     VALU / DPP / LDS work is spent on activation sums (the matrix pipe is idle anyway).
//   * activations: two 16-B loads per thread per 128-deep chunk, two chunks ahead, through a
//     double-buffered XOR-swizzled LDS tile (conflict-free ds_read_b128 fragments).  Deliberately
//     NOT LDS-DMA here: hipcc's s_waitcnt insertion cannot count DMA issued from inline asm, and an
//     over-estimated vmcnt wait on the weight ring is exactly what bounded the previous kernels
//     (weights effectively prefetched ~1 chunk ahead = an exposed HBM round trip per chunk, the
//     same 25-30 us on gate_up whatever the split-K or the instruction count).  With every VMEM
//     operation visible to the compiler all waits are exact counted vmcnt.
//   * weights: 16-B loads, 4-chunk register ring, refilled right after use (8 KiB per wave in
//     flight; HBM latency x 7 TB/s needs ~14 MB in flight chip-wide).
// Numerics are those of the general kernel's post-scaled path (fp32 accumulate of exact products,
// affine correction in fp32): within the GEMM tolerance of the reference tests
// (marlin_gemm_test.py:104-107), not bit-identical to "dequantise to T, then multiply".
//
// The main loop -- staging rings, pinned load order, unpack / MFMA / post-scale -- is w4_stream32.h, shared
// with the grouped MoE kernel (w4_moe.hip), which is the same stream over gathered rows; this file is its
// dense instance: index decode, row clamp, split-K bounds and the bias / split-K / SiLU epilogue.
#include "w4_plan.h"
#include "w4_stream32.h"

namespace slm {

// NG / SPAN: w4_stream32.h (scale groups per 128-deep chunk; groups wider than a chunk)
template <typename T, int NG, bool SPAN>
__global__ void __launch_bounds__(256, 2) w4a16_gemm_small_kernel(const GemmKParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bid = blockIdx.x;
  const int nb = bid % p.n_nblocks;
  bid /= p.n_nblocks;
  const int mb = bid % p.n_mblocks;
  const int ks = bid / p.n_mblocks;
  const int64_t m0 = (int64_t)mb * 32;
  const int64_t n_tiles = p.N / 32;
  int64_t nt = (int64_t)nb * 4 + wave;
  const bool nvalid = nt < n_tiles;
  if (!nvalid) nt = n_tiles - 1;  // clamped duplicate work, never stored

  const int c0 = ks * p.chunks_per_split;
  const int c1 = min(p.n_chunks, c0 + p.chunks_per_split);

  // ---- A: this thread's two (row, 16-B slot) sources of a chunk; rows >= M: clamped loads, never stored ----
  const char* abase = reinterpret_cast<const char*>(p.a);
  const char* a_src[2];
  int a_dst[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int idx = tid + 256 * i;
    const int row = idx >> 4, slot = idx & 15;
    const int64_t m = m0 + row;
    const int64_t mc = m < p.M ? m : p.M - 1;
    a_src[i] = abase + 2 * (mc * p.lda + slot * 8);
    a_dst[i] = stage_swz(row, slot);
  }
  const char* wlane = reinterpret_cast<const char*>(p.wq + (nt * 64 + lane) * 4);
  const char* szlane = reinterpret_cast<const char*>(p.sz + nt * 32 + (lane & 31));
  const uint32_t wstride = (uint32_t)(n_tiles * 1024);  // bytes per 64-deep half chunk
  const uint32_t szstride = (uint32_t)(p.N * 4);        // bytes per scale group
  const f32x16 acc = w4_stream32<T, NG, SPAN>(smem, a_src, a_dst, wlane, szlane, wstride, szstride,
                                              w4_cpg_shift(p.gs_shift), c0, c1, lane & 31, lane >> 5);

  // ---- epilogue: C/D layout of the 32x32 MFMA: col = lane & 31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).  Kept local
  // and written out: with the shared cd_store / cd_silu_exchange of w4_epilogue.h gate_up at M = 32 measured 2.6 %
  // slower, and with only the row through cd_row() still 3.9 % (hipcc schedules the whole kernel differently)
  const int64_t ncol = nt * 32 + (lane & 31);
  float bv = 0.f;
  if (p.split_k == 1 && p.bias) {
    const uint16_t braw = reinterpret_cast<const uint16_t*>(p.bias)[ncol];
    bv = lo_f32<T>((uint32_t)braw);
  }
  if (p.silu && p.split_k == 1) {
    // SLM_W4_SILU_MUL: waves (0, 1) and (2, 3) hold a (gate, up) tile pair.  The up wave hands its
    // T-rounded tile to the gate wave through the (now idle) A buffers; same lane, same r.
    uint16_t* ex = reinterpret_cast<uint16_t*>(smem) + (wave >> 1) * 1024;
    if (wave & 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) ex[r * 64 + lane] = pack1<T>(acc[r] + bv);
    }
    __syncthreads();
    if ((wave & 1) || !nvalid) return;
    const int64_t ocol = (nt >> 1) * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = m0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      const float g = lo_f32<T>((uint32_t)pack1<T>(acc[r] + bv));
      const float u = lo_f32<T>((uint32_t)ex[r * 64 + lane]);
      if (row < p.M) reinterpret_cast<uint16_t*>(p.c)[row * p.ldc + ocol] = pack1<T>(silu_mul1(g, u));
    }
    return;
  }
  if (!nvalid) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = m0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row < p.M) {
      if (p.split_k == 1)
        reinterpret_cast<uint16_t*>(p.c)[row * p.ldc + ncol] = pack1<T>(acc[r] + bv);
      else
        p.part[((int64_t)ks * p.M + row) * p.N + ncol] = acc[r];
    }
  }
}

template <typename T, int NG, bool SPAN>
static void launch_small_t(const GemmKParams& kp, int n_blocks, hipStream_t st) {
  hipLaunchKernelGGL((w4a16_gemm_small_kernel<T, NG, SPAN>), dim3((unsigned)n_blocks), dim3(256),
                     S32_LDS_BYTES, st, kp);
}

template <typename T>
static void launch_small_ng(const GemmKParams& kp, int ng, int n_blocks, hipStream_t st) {
  if (ng == 4) launch_small_t<T, 4, false>(kp, n_blocks, st);
  else if (ng == 2) launch_small_t<T, 2, false>(kp, n_blocks, st);
  else if (kp.gs_shift == 7) launch_small_t<T, 1, false>(kp, n_blocks, st);  // group 128
  else launch_small_t<T, 1, true>(kp, n_blocks, st);
}

void launch_gemm_small(const GemmKParams& kp, int dtype, const GemmPlan& pl, hipStream_t st) {
  dispatch_dtype(dtype, [&](auto t) { launch_small_ng<decltype(t)>(kp, pl.ng, pl.n_blocks(), st); });
}

}  // namespace slm
