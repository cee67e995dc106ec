// moe_gemm_plan.h -- the chunk / ring constants and the launch shape of moe_gemm.hip's grouped GEMMs over
// checkpoint-layout experts.
#pragma once
#include "common.h"

namespace slm {

constexpr int MG_RING = 3;                // weight / A register rings (chunks)
constexpr int MG_KC = 128;                // k per chunk
constexpr int MG_STAGE_BYTES = 32 * 256;  // one chunk of A: 32 rows x 128 k
constexpr int MG_LDS_BYTES = 2 * MG_STAGE_BYTES;

// Waves (adjacent 32-column tiles) per workgroup: the widest of 4, 2, 1 that still yields one workgroup
// per CU, otherwise the narrowest.  SiLU * mul pairs waves, so it never goes below 2.  Decided from the
// arguments alone: the same call always launches the same shape.
static int moe_gemm_waves(int64_t max_blocks, int64_t n_tiles, bool silu) {
  const int narrowest = silu ? 2 : 1;
  for (int nw = 4; nw > narrowest; nw >>= 1)
    if (max_blocks * gemm_col_groups(n_tiles, nw, silu) >= MI355X_CUS) return nw;
  return narrowest;
}

}  // namespace slm
