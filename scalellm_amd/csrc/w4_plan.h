// w4_plan.h -- the launch plan of slm_w4a16_gemm: which of the eight kernels takes a call, and with what
// grid.  w4_plan.hip decides (host code only, no HIP call), w4.hip's gemm_impl switches on the result, the
// launch_* functions of the kernel files read their own part of it.
#pragma once
#include "w4_common.h"

namespace slm {

enum class W4Kernel : int {  // (public mirror: slm_w4_kernel, include/slm_hip.h -- same order)
  GEMV,     // w4_gemv.hip     dot2 GEMV, M <= 4, K split inside the workgroup
  KS,       // w4_ks.hip       K-sliced weight stream: one row tile (M <= 32) or two (33 <= M <= 64)
  SMALL,    // w4_small.hip    lean weight stream, M <= 32 (where the K-sliced kernel steps aside)
  GENERAL,  // w4_general.hip  32 / 64 / 128-row tiles
  M128,     // w4_m128.hip     65 <= M <= 128, all rows in one workgroup
  WS,       // w4_ws.hip       wave-specialised 256 x 128 tiles
  XL,       // w4_xl.hip       symmetric 256 x 256 tiles
  XL_SK,    // w4_xl.hip       ... stream-K form: the tile x K work cut into equal ranges
};

struct GemmPlan {
  W4Kernel kernel;
  int ng;                // scale groups per 128-deep chunk (1 for group >= 128, 2 for 64, 4 for 32)
  int split_k, chunks_per_split, n_mblocks, n_nblocks;
  size_t lds_bytes;      // dynamic LDS of the launch (GEMV: + one fp32 row with the norm prologue)
  size_t part_bytes, aperm_bytes;  // workspace: fp32 partials, then the act-order copy of A
  // one struct per kernel that has parameters of its own: its planner fills it, its launch reads it, the
  // others stay zero
  struct { int mt, ntw, pc, post; } general;  // row tiles, column tiles per wave, chunks per pass, post-scaled form
  struct { int mt, cw, nw, tpw; } ks;         // row tiles, chunks of K per wave, waves, column tiles per workgroup
  struct { int wd, kw, ct, adma; } m128;      // weight ring depth, waves per column tile, column tiles, LDS-DMA A
  struct { int sk_per; } xl_sk;               // 128-deep chunks of the work list per workgroup
  int n_blocks() const { return n_nblocks * n_mblocks * split_k; }
};

// SLM_OK and *pl, or why `a` cannot run; M == 0 plans like any other call
int plan_gemm(const slm_w4_gemm_args* a, GemmPlan* pl);

void launch_gemv(const GemmKParams& kp, int dtype, const GemmPlan& pl, hipStream_t st);
void launch_gemm_ks(const GemmKParams& kp, int dtype, const GemmPlan& pl, hipStream_t st);
void launch_gemm_small(const GemmKParams& kp, int dtype, const GemmPlan& pl, hipStream_t st);
void launch_gemm_general(const GemmKParams& kp, int dtype, const GemmPlan& pl, hipStream_t st);
void launch_gemm_m128(const GemmKParams& kp, int dtype, const GemmPlan& pl, hipStream_t st);
void launch_gemm_ws(const GemmKParams& kp, int dtype, const GemmPlan& pl, hipStream_t st);
void launch_gemm_xl(const GemmKParams& kp, int dtype, const GemmPlan& pl, hipStream_t st);
void launch_gemm_xl_sk(const GemmKParams& kp, int dtype, const GemmPlan& pl, hipStream_t st);

}  // namespace slm
