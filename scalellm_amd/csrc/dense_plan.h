// dense_plan.h -- the launch plan of dense.hip's three entries (slm_linear, slm_fp8_linear, slm_mxfp4_linear;
// include/slm_hip.h sections 13, 15 and 20), over any of the argument structs: slm_fp8_linear_args and
// slm_mxfp4_linear_args are slm_linear_args, field for field, plus their scales.  Host only.
#pragma once
#include "common.h"
#include "tuning.h"

namespace slm {

constexpr int LIN_KC = 128;   // k per chunk
constexpr int LIN_MAX_SPLIT = 16;

// ---- the plan: a pure host function of (M, N, K, dtype, flags, bias != NULL, tuning table) ----
struct LinearPlan {
  int rt, nw;
  int64_t row_blocks, col_groups;
  int split_k, n_chunks, tail_units;
  int slice_chunk[LIN_MAX_SPLIT + 1];
  uint64_t lds_bytes, ws_bytes;
};

template <typename Args>
inline int plan_linear(const Args* a, LinearPlan* pl) {
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

}  // namespace slm
