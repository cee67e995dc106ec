// w4_epilogue.h -- the epilogues of the MFMA GEMM kernels, one per accumulator layout.
//
// C/D layout (w4_general, w4_m128, w4_moe; w4_small and moe_gemm keep their own, written out: see there): a
// wave's 32 x 32 tile sits with column = lane & 31 and row = cd_row(r, lane) in accumulator register r.  cd_store
// writes a column tile of MT row tiles as T(acc + bias) to c, cd_store_splitk that or fp32 to a split-K slab;
// cd_silu_exchange is SLM_W4_SILU_MUL over a (gate, up) pair of waves.  Where a row goes is the row map's
// business: dense rows (DenseRows) or the scatter of the grouped int4 MoE GEMM (ScatterRows), which takes no bias
// and may scale a row before the rounding.
//
// C^T layout (w4_ws, w4_xl: the MFMAs ran with the operands swapped): lane = token, the 16 registers are the
// columns 8 (r >> 2) + 4 (lane >> 5) + (r & 3) -- four consecutive columns per r >> 2, one 8-byte (T) or 16-byte
// (fp32 slab) store.  ct_store is that epilogue for a wave's two adjacent column tiles.
//
// Every arithmetic expression here is pinned bit for bit by the exact tests (tests/test_w4_exact_gpu.py,
// test_moe_dense_gpu.py): RNE_T(sum + bias), RNE_T(silu_mul1(RNE_T(gate), RNE_T(up))).
#pragma once
#include "w4_common.h"

namespace slm {

// row of accumulator register r inside the 32 x 32 C/D tile: a part fixed by r plus a part fixed by the lane
__device__ __forceinline__ int cd_row_reg(int r) { return (r & 3) + 8 * (r >> 2); }
__device__ __forceinline__ int cd_row_lane(int lane) { return 4 * (lane >> 5); }
__device__ __forceinline__ int cd_row(int r, int lane) { return cd_row_reg(r) + cd_row_lane(lane); }

// bias of column `col` (T) as fp32, 0 without a bias vector
template <typename T>
__device__ __forceinline__ float cd_bias(const void* bias, int64_t col) {
  return bias ? lo_f32<T>((uint32_t)reinterpret_cast<const uint16_t*>(bias)[col]) : 0.f;
}

// Row maps: (row tile m, register r) of this lane -> `row` of c; false: do not store.
struct DenseRows {  // rows m0 .. of an [M, ldc] matrix
  static constexpr bool scattered = false;
  int64_t m0, M;
  __device__ __forceinline__ bool operator()(int m, int r, int lane, int64_t& row) const {
    // (summed in this order: the compile-time part folds into the addressing; with cd_row() as one 32-bit term
    // hipcc keeps two more VGPRs live through the main loop of some w4_general instantiations)
    row = m0 + (m * 32 + cd_row_reg(r)) + cd_row_lane(lane);
    return row < M;
  }
};
struct ScatterRows {  // the block's flat indices (LDS, written before the first barrier); padding is >= n_flat
  static constexpr bool scattered = true;
  const int* s_idx;
  int n_flat;
  const float* row_scale;  // [n_flat] or NULL: a factor on the row before the rounding (plain store only)
  __device__ __forceinline__ bool operator()(int m, int r, int lane, int64_t& row) const {
    const int fi = s_idx[m * 32 + cd_row(r, lane)];
    row = fi;
    return (unsigned)fi < (unsigned)n_flat;
  }
};

// acc + bias where the layout has a bias (the grouped GEMMs have none: not even + 0, which would turn -0 into +0)
template <typename RowMap>
__device__ __forceinline__ float cd_biased(float acc, float bv) {
  if constexpr (RowMap::scattered) return acc;
  else return acc + bv;
}

// Column tile `tile` (column 32 tile + (lane & 31) in this lane) of MT row tiles of a kernel with split-K.
// final_out (split_k == 1): T(acc + bv) -> c[row, col], a scattered row first times the map's row_scale[row];
// otherwise fp32 -> part[slab_row0 + row, col] of the [split_k * M, N] slabs.  One loop with the branch inside, as the
// kernels had it: hoisted into two loops, the four-row-tile general kernel spills 54 SGPRs.
template <typename T, int MT, typename RowMap>
__device__ __forceinline__ void cd_store_splitk(const f32x16 (&acc)[MT], const RowMap& rows, const int lane,
                                                const bool final_out, void* c, const int64_t ldc, const int64_t tile,
                                                const float bv, float* part, const int64_t slab_row0, const int64_t N) {
  const int64_t col = tile * 32 + (lane & 31);
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int64_t row;
      if (rows(m, r, lane, row)) {
        if (final_out) {
          float v = cd_biased<RowMap>(acc[m][r], bv);
          if constexpr (RowMap::scattered) {
            if (rows.row_scale) v *= rows.row_scale[row];
          }
          reinterpret_cast<uint16_t*>(c)[row * ldc + col] = pack1<T>(v);
        } else {
          part[(slab_row0 + row) * N + col] = acc[m][r];
        }
      }
    }
  }
}
// ... of a kernel without split-K
template <typename T, int MT, typename RowMap>
__device__ __forceinline__ void cd_store(const f32x16 (&acc)[MT], const RowMap& rows, const int lane, void* c,
                                         const int64_t ldc, const int64_t tile, const float bv) {
  cd_store_splitk<T, MT>(acc, rows, lane, true, c, ldc, tile, bv, nullptr, 0, 0);
}

// The store loop of SLM_W4_SILU_MUL: g = this wave's T-rounded gate value, up_t(m, r) = the T-rounded up value
// of the same (lane, m, r) as fp32;  T(silu_mul1(g, u)) -> c[row, ocol]
template <typename T, int MT, typename RowMap, typename UpFn>
__device__ __forceinline__ void cd_store_silu(const f32x16 (&gate)[MT], const float bg, const UpFn& up_t,
                                              const RowMap& rows, const int lane, void* c, const int64_t ldc,
                                              const int64_t ocol) {
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int64_t row;
      const bool on = rows(m, r, lane, row);
      const float g = lo_f32<T>((uint32_t)pack1<T>(cd_biased<RowMap>(gate[m][r], bg)));
      const float u = up_t(m, r);
      if (on) reinterpret_cast<uint16_t*>(c)[row * ldc + ocol] = pack1<T>(silu_mul1(g, u));
    }
  }
}

// SLM_W4_SILU_MUL over a pair of waves holding the (gate, up) tiles of one output tile: the up wave hands its
// T-rounded tile to the gate wave through `ex` (the pair's MT * 1024 uint16 of the now idle A buffers; same
// lane, same (m, r)).  Called by EVERY wave of the workgroup -- the barrier is in here; `up` / `gate` say what
// this wave is (neither: a wave that only meets the barrier; a clamped gate tile computes but is no `gate`).
// bias (NULL: none) is read at this wave's own column tile `tile`; otile: the pair's column tile of c.
template <typename T, int MT, typename RowMap>
__device__ __forceinline__ void cd_silu_exchange(const f32x16 (&acc)[MT], const RowMap& rows, const int lane,
                                                 uint16_t* ex, const bool up, const bool gate, const void* bias,
                                                 const int64_t tile, void* c, const int64_t ldc, const int64_t otile) {
  if (up) {
    const float bv = cd_bias<T>(bias, tile * 32 + (lane & 31));
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) ex[(m * 16 + r) * 64 + lane] = pack1<T>(cd_biased<RowMap>(acc[m][r], bv));
  }
  __syncthreads();
  if (!gate) return;
  const int64_t ocol = otile * 32 + (lane & 31);
  const float bv = cd_bias<T>(bias, tile * 32 + (lane & 31));
  cd_store_silu<T, MT>(acc, bv, [&](int m, int r) { return lo_f32<T>((uint32_t)ex[(m * 16 + r) * 64 + lane]); }, rows,
                       lane, c, ldc, ocol);
}

// ------------------------------------------------------------------------------------------
// C^T layout
// ------------------------------------------------------------------------------------------
// SLM_W4_SILU_MUL epilogue of the C^T-accumulator kernels (split_k == 1):
// the wave's two adjacent column tiles t0 (even: gate) and t0 + 1 (up) sit in the same lane at the
// same (i, r), so the pair never leaves its registers.  Lane = token row0 + 32 i; the 16 values
// are the columns (r & 3) + 8 (r >> 2) + 4 (lane >> 5): four consecutive outputs per r >> 2.
template <typename T>
__device__ __forceinline__ void store_ct_silu_pair(const GemmKParams& p, const f32x16 (&acc)[2][4],
                                                   const int64_t t0, const int64_t row0,
                                                   const int lane) {
  if ((t0 + 1) * 32 >= p.N) return;
  const bool wide = ((p.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(p.c) & 7) == 0);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t gcol = t0 * 32 + 8 * q + 4 * (lane >> 5);
    const int64_t ocol = (t0 >> 1) * 32 + 8 * q + 4 * (lane >> 5);
    float bg[4] = {0.f, 0.f, 0.f, 0.f}, bu[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) {
      const uint16_t* bp = reinterpret_cast<const uint16_t*>(p.bias) + gcol;
      const u32x2 g = *reinterpret_cast<const u32x2*>(bp);
      const u32x2 u = *reinterpret_cast<const u32x2*>(bp + 32);
      bg[0] = lo_f32<T>(g.x); bg[1] = hi_f32<T>(g.x); bg[2] = lo_f32<T>(g.y); bg[3] = hi_f32<T>(g.y);
      bu[0] = lo_f32<T>(u.x); bu[1] = hi_f32<T>(u.x); bu[2] = lo_f32<T>(u.y); bu[3] = hi_f32<T>(u.y);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = row0 + i * 32;
      if (row >= p.M) continue;
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        o[e] = silu_mul_acc<T>(acc[0][i][4 * q + e] + bg[e], acc[1][i][4 * q + e] + bu[e]);
      uint16_t* dst = reinterpret_cast<uint16_t*>(p.c) + row * p.ldc + ocol;
      u32x2 w;
      w.x = pack2<T>(o[0], o[1]);
      w.y = pack2<T>(o[2], o[3]);
      if (wide) {
        *reinterpret_cast<u32x2*>(dst) = w;
      } else {
        dst[0] = (uint16_t)(w.x & 0xffffu); dst[1] = (uint16_t)(w.x >> 16);
        dst[2] = (uint16_t)(w.y & 0xffffu); dst[3] = (uint16_t)(w.y >> 16);
      }
    }
  }
}

// A wave's two adjacent column tiles t0, t0 + 1 over the four row tiles row0 + 32 i (row0 includes lane & 31).
// final_out = true: T(acc + bias) into c (SLM_W4_SILU_MUL: the pair above);  false: fp32 into the split-K slab
// `ks` of p.part
template <typename T>
__device__ __forceinline__ void ct_store(const GemmKParams& p, const f32x16 (&acc)[2][4], const int64_t t0,
                                         const int64_t row0, const int lane, const int ks, const bool final_out) {
  if (p.silu && final_out) {
    store_ct_silu_pair<T>(p, acc, t0, row0, lane);
    return;
  }
  const int64_t n_tiles = p.N / 32;
  const bool wide = ((p.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(p.c) & 7) == 0);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t t = t0 + j;
    if (t >= n_tiles) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t ncol = t * 32 + 8 * q + 4 * (lane >> 5);
      float bv[4] = {0.f, 0.f, 0.f, 0.f};
      if (final_out && p.bias) {
        const u32x2 b = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(p.bias) + ncol);
        bv[0] = lo_f32<T>(b.x); bv[1] = hi_f32<T>(b.x);
        bv[2] = lo_f32<T>(b.y); bv[3] = hi_f32<T>(b.y);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = row0 + i * 32;
        if (row >= p.M) continue;
        const float v0 = acc[j][i][4 * q + 0], v1 = acc[j][i][4 * q + 1];
        const float v2 = acc[j][i][4 * q + 2], v3 = acc[j][i][4 * q + 3];
        if (final_out) {
          uint16_t* dst = reinterpret_cast<uint16_t*>(p.c) + row * p.ldc + ncol;
          u32x2 o;
          o.x = pack2<T>(v0 + bv[0], v1 + bv[1]);
          o.y = pack2<T>(v2 + bv[2], v3 + bv[3]);
          if (wide) {
            *reinterpret_cast<u32x2*>(dst) = o;
          } else {
            dst[0] = (uint16_t)(o.x & 0xffffu); dst[1] = (uint16_t)(o.x >> 16);
            dst[2] = (uint16_t)(o.y & 0xffffu); dst[3] = (uint16_t)(o.y >> 16);
          }
        } else {
          const f32x4 o = {v0, v1, v2, v3};
          *reinterpret_cast<f32x4*>(p.part + ((int64_t)ks * p.M + row) * p.N + ncol) = o;
        }
      }
    }
  }
}

}  // namespace slm
