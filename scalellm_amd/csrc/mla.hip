// mla.hip -- multi-head latent attention (MLA) over a paged latent KV cache, and the latent cache append.
//
// Semantics (reference tests/mla_ref.h, kernel family src/kernels/attention/device/sm80_mla_dispatch.cuh,
// parameters mla_params.h), per sequence b and head h:
//   S[q, k]    = sm_scale * (q[q,h,:] . kv[k,:] + q_rope[q,h,:] . k_rope[k,:])
//   S[q, k]    = -inf where k > q + (kv_len_b - q_len_b)
//   out[q,h,:] = softmax_k(S[q,:]) . kv[:, :]            (V IS the latent row)
// One latent row [head_dim] and one RoPE key [rope_head_dim = 64] per token, shared by ALL heads; both
// caches paged as in attention (slot = table[bcu[b] + (i >> log2 bs)] + (i & (bs - 1))).
//
// Work item: one workgroup of FOUR waves = (sequence, tile of 32 NQ query rows, KV split); a query row
// is a (token, head) pair with the head fastest, so a tile may hold rows of several tokens, each with
// its own causal limit (row -> token is row / n_heads).  The workgroup walks its KV range in tiles of
// 32 tokens.  ONE LDS image of the tile serves both products:
//
//   image: (head_dim + 64) / 16 sub-tiles of [32 kv][16 d] (32 B per kv row, 1 KiB per sub-tile; the
//          image attn_tile.hip keeps V in), the RoPE key's four sub-tiles behind the latent's.
//   S^T[32 kv x 32 q] = K . Q^T   the contraction over head_dim + 64 is SPLIT ACROSS THE WAVES: wave w
//          takes the sub-tiles [w NSUB/4, (w+1) NSUB/4) -- one sub-tile is one k-step of
//          v_mfma_f32_32x32x16, its A fragment one linear, conflict-free 1 KiB ds_read_b128 (lane ->
//          kv row lane % 32, 16-B half lane / 32) -- and holds only THOSE dims of Q in registers (36
//          VGPRs per 32 rows at 512 + 64 instead of 144).  The four partial blocks meet in LDS (fp32,
//          16 KiB per 32 rows); every wave adds them in the same order, so all four hold the same
//          bits and run the same online softmax.
//   O^T[d x 32 q] += V^T . P^T   the output width is split across the waves: wave w owns the columns
//          [w head_dim/4, (w+1) head_dim/4): head_dim/128 accumulator tiles of 16 registers per 32
//          rows.  A = V^T comes out of the same image by ds_read_b64_tr_b16; B = P straight from the
//          softmax registers (the C-fragment row order is the contraction order, as in attn_tile.hip).
//
// The next tile travels HBM -> registers while this one is consumed; three barriers per tile (partial
// scores published / tile consumed / next tile stored).  Split-KV: fp32 partials and (m, l) through the
// caller's workspace, merged by mla_combine_kernel in a fixed order (no atomics: repeats are
// bit-identical; a split without KV tokens publishes l = 0 and merges as a no-op).
#include "attn_common.h"

namespace slm {

namespace {

struct MlaKParams {
  void* out;
  const void* q;
  const void* q_rope;
  const void* kvc;
  const void* krc;
  int64_t o_ts, o_hs, q_ts, q_hs, qr_ts, qr_hs, kv_ss, kr_ss;  // strides in elements
  const int* q_cu;
  const int* kv_cu;
  const int* bt;
  const int* bcu;
  float* o_part;   // [n_tokens, n_heads, n_splits, head_dim]
  float* ml_part;  // [n_tokens, n_heads, n_splits, 2]
  int batch, n_heads;
  int block_shift, block_mask;
  int n_splits, tiles_per_seq;
  float scale_log2;  // sm_scale * log2(e)
};

constexpr int MLA_ROPE = 64;
constexpr int MLA_WAVES = 4;
constexpr int MLA_TILE_KV = 32;
constexpr int MLA_SUB_STRIDE = 1280;  // a 1 KiB sub-tile + 256 B: see mla_sub_base
// Sub-tile s of the image: the padding rotates the sub-tiles over the banks exactly as attn_tile.hip's
// v_sub_base does (an odd sub-tile lands 32 banks from its even partner, which is what the two 16-lane
// groups of a transpose-read phase touch), with the rotation taken mod 8 so that it stays inside the
// 256 B of padding for any number of sub-tiles.
__device__ __forceinline__ constexpr int mla_sub_base(int s) {
  return s * MLA_SUB_STRIDE + 32 * (((s >> 1) & 3) + 4 * (s & 1));
}
typedef short tr_v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) tr_v4s tr_lds_v4s;

// NQ: 32-row query blocks per workgroup (1: up to 32 rows -- decode with few heads; 2: 64 rows).
template <typename T, int HD, int NQ>
__global__ void __launch_bounds__(64 * MLA_WAVES) __attribute__((amdgpu_waves_per_eu(HD * NQ >= 1024 ? 1 : 2))) mla_kernel(const MlaKParams p) {
  typedef typename Mfma<T>::frag frag_t;
  constexpr int NSUB = (HD + MLA_ROPE) / 16;     // sub-tiles = k-steps of the score product
  constexpr int NSUB_KV = HD / 16;               // ... of which the latent's
  constexpr int KS = NSUB / MLA_WAVES;           // k-steps per wave
  constexpr int DTW = HD / (32 * MLA_WAVES);     // 32-column output tiles per wave
  constexpr int NSLOT = (HD + MLA_ROPE) / 8;     // 16-B slots per token (latent, then RoPE key)
  constexpr int NSLOT_KV = HD / 8;
  constexpr int NT = 64 * MLA_WAVES;
  constexpr int ITEMS = MLA_TILE_KV * NSLOT / NT;   // 16-B staging items per thread and tile: ITEMS - 1 latent, 1 RoPE
  constexpr int TILE_BYTES = NSUB * MLA_SUB_STRIDE;
  static_assert(NSUB % MLA_WAVES == 0 && HD % (32 * MLA_WAVES) == 0, "the waves split both products evenly");
  static_assert((MLA_TILE_KV * NSLOT_KV) % NT == 0 && NT % NSLOT_KV == 0 && MLA_TILE_KV * (MLA_ROPE / 8) == NT,
                "whole staging items per thread");
  __shared__ __attribute__((aligned(16))) char kv_lds[TILE_BYTES];
  __shared__ __attribute__((aligned(16))) float sx[MLA_WAVES * NQ * 16 * 64];   // the waves' partial score blocks

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5;
  const int l31 = lane & 31;

  int bid = blockIdx.x;
  const int split = bid % p.n_splits;
  bid /= p.n_splits;
  const int tile = bid % p.tiles_per_seq;
  const int b = bid / p.tiles_per_seq;

  const int q_start = p.q_cu[b];
  const int q_len = p.q_cu[b + 1] - q_start;
  const int kv_len = p.kv_cu[b + 1] - p.kv_cu[b];
  const int G = p.n_heads;
  const int rows_total = q_len * G;
  constexpr int ROWS = 32 * NQ;
  const int row0 = tile * ROWS;
  if (row0 >= rows_total) return;  // workgroup-uniform

  // this lane's query rows (one per 32-row block)
  bool jvalid[NQ];
  int tq[NQ], head[NQ], diag[NQ];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    const int jrow = row0 + 32 * n + l31;
    jvalid[n] = jrow < rows_total;
    tq[n] = jvalid[n] ? jrow / G : (rows_total - 1) / G;
    head[n] = jvalid[n] ? jrow % G : 0;
    diag[n] = kv_len - q_len + tq[n];  // last visible kv index of this row (causal, bottom-right aligned)
  }

  // Q fragments (B operand of S^T = K . Q^T) of THIS wave's k-steps: 8 consecutive dims per lane and step
  frag_t qf[NQ][KS];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    const char* qp = reinterpret_cast<const char*>(p.q) +
                     2 * ((int64_t)(q_start + tq[n]) * p.q_ts + (int64_t)head[n] * p.q_hs + 8 * hh);
    const char* qrp = reinterpret_cast<const char*>(p.q_rope) +
                      2 * ((int64_t)(q_start + tq[n]) * p.qr_ts + (int64_t)head[n] * p.qr_hs + 8 * hh);
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int s = wave * KS + j;  // (wave-uniform)
      const char* src = s < NSUB_KV ? qp + 32 * s : qrp + 32 * (s - NSUB_KV);
      u32x4 v = {0u, 0u, 0u, 0u};
      if (jvalid[n]) v = *reinterpret_cast<const u32x4*>(src);
      qf[n][j] = __builtin_bit_cast(frag_t, v);
    }
  }

  // KV range of the workgroup: the causal bound of its last row; a split's share in whole tiles
  // (trailing splits may be empty: they publish l = 0)
  const int last_row = min(row0 + ROWS, rows_total) - 1;
  const int wg_hi = max(0, min(kv_len, kv_len - q_len + last_row / G + 1));
  int wg_lo = 0, wg_hi_s = wg_hi;
  if (p.n_splits > 1) {
    const int n_t = (wg_hi + MLA_TILE_KV - 1) / MLA_TILE_KV;
    const int per = ((n_t + p.n_splits - 1) / p.n_splits) * MLA_TILE_KV;
    wg_lo = min(split * per, wg_hi);
    wg_hi_s = min(wg_hi, wg_lo + per);
  }

  f32x16 oacc[NQ][DTW];
  float m_run[NQ], l_run[NQ];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    m_run[n] = ATTN_M_INIT;
    l_run[n] = 0.f;
#pragma unroll
    for (int d = 0; d < DTW; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[n][d][r] = 0.f;
  }

  const int bcu0 = p.bcu[b];
  const char* kvbase = reinterpret_cast<const char*>(p.kvc);
  const char* krbase = reinterpret_cast<const char*>(p.krc);
  const uint64_t kv_sb = (uint64_t)(2 * p.kv_ss), kr_sb = (uint64_t)(2 * p.kr_ss);

  // Staging: 16 B per lane and item.  Latent items and RoPE-key items are separate (which cache an item reads
  // is then a compile-time fact, not a per-lane choice): latent item i of a thread is slot tid % NSLOT_KV of tile
  // row tid / NSLOT_KV + (NT / NSLOT_KV) i; the one RoPE item is slot tid % 8 of row tid / 8.
  constexpr int ROWS_PER_PASS = NT / NSLOT_KV;
  int sreg[ITEMS];     // cache slots of the rows of the next tile_load (the last one: the RoPE item's)
  u32x4 treg[ITEMS];   // the tile in flight
  const int kv_r0 = tid / NSLOT_KV, kv_sl = tid % NSLOT_KV;
  const int kr_r = tid >> 3, kr_sl = tid & 7;
  auto slot_of = [&](int row) {
    row = min(row, wg_hi_s - 1);  // clamp: masked below, must stay inside the sequence
    return p.bt[bcu0 + (row >> p.block_shift)] + (row & p.block_mask);
  };
  auto slot_load = [&](int kt0) {
#pragma unroll
    for (int i = 0; i < ITEMS - 1; ++i) sreg[i] = slot_of(kt0 + kv_r0 + ROWS_PER_PASS * i);
    sreg[ITEMS - 1] = slot_of(kt0 + kr_r);
  };
  auto tile_load = [&]() {
#pragma unroll
    for (int i = 0; i < ITEMS - 1; ++i)
      treg[i] = *reinterpret_cast<const u32x4*>(kvbase + (uint64_t)(uint32_t)sreg[i] * kv_sb + 16 * kv_sl);
    treg[ITEMS - 1] = *reinterpret_cast<const u32x4*>(krbase + (uint64_t)(uint32_t)sreg[ITEMS - 1] * kr_sb + 16 * kr_sl);
  };
  auto tile_store = [&]() {
#pragma unroll
    for (int i = 0; i < ITEMS - 1; ++i)
      *reinterpret_cast<u32x4*>(kv_lds + mla_sub_base(kv_sl >> 1) + (kv_r0 + ROWS_PER_PASS * i) * 32 + ((kv_sl & 1) << 4)) = treg[i];
    *reinterpret_cast<u32x4*>(kv_lds + mla_sub_base(NSUB_KV + (kr_sl >> 1)) + kr_r * 32 + ((kr_sl & 1) << 4)) = treg[ITEMS - 1];
  };
  // transpose-read address of this lane inside a sub-tile pair (as in attn_tile.hip): lanes 16..31 / 48..63
  // read the odd sub-tile (columns 16..31 of the 32-column tile), the upper lane half kv rows + 4
  const uint32_t v_lane = (uint32_t)(uintptr_t)kv_lds +
                          (uint32_t)(((lane & 15) >> 2) * 32 + (lane & 3) * 8 + hh * 128 +
                                     ((lane >> 4) & 1) * (mla_sub_base(1) - mla_sub_base(0)));
  const int k_lane = l31 * 32 + hh * 16;   // row-read address inside a sub-tile: K[kv = l31][8 hh .. 8 hh + 7]

  if (wg_lo < wg_hi_s) {   // (workgroup-uniform: every barrier below is reached by all or by none)
    slot_load(wg_lo);
    tile_load();
    slot_load(wg_lo + MLA_TILE_KV);
    tile_store();
    __syncthreads();
    for (int kt0 = wg_lo; kt0 < wg_hi_s; kt0 += MLA_TILE_KV) {
      const bool more = kt0 + MLA_TILE_KV < wg_hi_s;
      if (more) {  // next tile HBM -> registers, then the slots of the one after
        tile_load();
        slot_load(kt0 + 2 * MLA_TILE_KV);
      }

      // ---- this wave's share of S^T = K . Q^T ----
      {
        f32x16 sp[NQ];
#pragma unroll
        for (int n = 0; n < NQ; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) sp[n][r] = 0.f;
#pragma unroll
        for (int j = 0; j < KS; ++j) {
          const int s = wave * KS + j;
          const u32x4 kv4 = *reinterpret_cast<const u32x4*>(kv_lds + mla_sub_base(s) + k_lane);
#pragma unroll
          for (int n = 0; n < NQ; ++n) sp[n] = Mfma<T>::run(__builtin_bit_cast(frag_t, kv4), qf[n][j], sp[n]);
        }
#pragma unroll
        for (int n = 0; n < NQ; ++n)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *reinterpret_cast<f32x4*>(sx + ((((wave * NQ + n) * 4 + g) * 64 + lane) << 2)) =
                f32x4{sp[n][4 * g + 0], sp[n][4 * g + 1], sp[n][4 * g + 2], sp[n][4 * g + 3]};
      }
      __syncthreads();

      // ---- the full block (same order of addition in every wave), mask, online softmax ----
      u32x4 pb[NQ][2];
#pragma unroll
      for (int n = 0; n < NQ; ++n) {
        float sc[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 a = *reinterpret_cast<const f32x4*>(sx + ((((0 * NQ + n) * 4 + g) * 64 + lane) << 2));
#pragma unroll
          for (int w = 1; w < MLA_WAVES; ++w) a += *reinterpret_cast<const f32x4*>(sx + ((((w * NQ + n) * 4 + g) * 64 + lane) << 2));
          sc[4 * g + 0] = a.x; sc[4 * g + 1] = a.y; sc[4 * g + 2] = a.z; sc[4 * g + 3] = a.w;
        }
        float mloc = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv_idx = kt0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
          const bool vis = jvalid[n] && kv_idx <= diag[n] && kv_idx < kv_len;
          const float a = vis ? sc[r] * p.scale_log2 : -INFINITY;
          sc[r] = a;
          mloc = fmaxf(mloc, a);
        }
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        // lazy reference update (attn_tile.hip): the running max only has to bound the exponents
        constexpr float LAZY_TH = 6.0f;
        if (__any(mloc > m_run[n] + LAZY_TH)) {
          const float m_new = fmaxf(m_run[n], mloc);
          const float alpha = fast_exp2(m_run[n] - m_new);
          m_run[n] = m_new;
          l_run[n] *= alpha;
#pragma unroll
          for (int d = 0; d < DTW; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[n][d][r] *= alpha;
        }
        float lsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sc[r] = fast_exp2(sc[r] - m_run[n]);
          lsum += sc[r];
        }
        lsum += __shfl_xor(lsum, 32, 64);
        l_run[n] += lsum;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          pb[n][s2].x = pack2<T>(sc[8 * s2 + 0], sc[8 * s2 + 1]);
          pb[n][s2].y = pack2<T>(sc[8 * s2 + 2], sc[8 * s2 + 3]);
          pb[n][s2].z = pack2<T>(sc[8 * s2 + 4], sc[8 * s2 + 5]);
          pb[n][s2].w = pack2<T>(sc[8 * s2 + 6], sc[8 * s2 + 7]);
        }
      }

      // ---- O^T += V^T . P^T over this wave's columns (all lanes active: the transpose read needs it) ----
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
        for (int d = 0; d < DTW; ++d) {
          const int dt = wave * DTW + d;   // 32-column tile of the output
          const uintptr_t va0 = v_lane + (uint32_t)(mla_sub_base(2 * dt) + 16 * s2 * 32);
          const tr_v4s t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_lds_v4s*)va0);
          const tr_v4s t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_lds_v4s*)(va0 + 8 * 32));
          const u32x2 v0 = __builtin_bit_cast(u32x2, t0), v1 = __builtin_bit_cast(u32x2, t1);
          const u32x4 va = {v0.x, v0.y, v1.x, v1.y};
#pragma unroll
          for (int n = 0; n < NQ; ++n)
            oacc[n][d] = Mfma<T>::run(__builtin_bit_cast(frag_t, va), __builtin_bit_cast(frag_t, pb[n][s2]), oacc[n][d]);
        }
      }
      if (more) {
        __syncthreads();   // every wave is done with this tile and with the partial scores
        tile_store();
        __syncthreads();
      }
    }
  }

  // ---- epilogue: O^T[d][q] -> out[token][head][d], 4 consecutive d per register quad ----
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    if (!jvalid[n]) continue;
    if (p.n_splits > 1) {
      const int64_t pi = ((int64_t)(q_start + tq[n]) * p.n_heads + head[n]) * p.n_splits + split;
      float* opp = p.o_part + pi * HD;
#pragma unroll
      for (int d = 0; d < DTW; ++d)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
          *reinterpret_cast<f32x4*>(opp + (wave * DTW + d) * 32 + 8 * q4 + 4 * hh) =
              f32x4{oacc[n][d][4 * q4 + 0], oacc[n][d][4 * q4 + 1], oacc[n][d][4 * q4 + 2], oacc[n][d][4 * q4 + 3]};
      if (wave == 0 && hh == 0) {
        p.ml_part[pi * 2 + 0] = m_run[n];
        p.ml_part[pi * 2 + 1] = l_run[n];
      }
      continue;
    }
    const float inv = l_run[n] > 0.f ? 1.0f / l_run[n] : 0.f;
    char* op = reinterpret_cast<char*>(p.out) + 2 * ((int64_t)(q_start + tq[n]) * p.o_ts + (int64_t)head[n] * p.o_hs);
#pragma unroll
    for (int d = 0; d < DTW; ++d)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int dd = (wave * DTW + d) * 32 + 8 * q4 + 4 * hh;
        u32x2 o2;
        o2.x = pack2<T>(oacc[n][d][4 * q4 + 0] * inv, oacc[n][d][4 * q4 + 1] * inv);
        o2.y = pack2<T>(oacc[n][d][4 * q4 + 2] * inv, oacc[n][d][4 * q4 + 3] * inv);
        *reinterpret_cast<u32x2*>(op + 2 * dd) = o2;
      }
  }
}

// out[row, :] = sum_s O_s 2^(m_s - M) / sum_s l_s 2^(m_s - M), M = max_s m_s, in split order.  One workgroup
// per (token, head) row, four columns per thread.  Rows past q_cu[batch] (graph padding) are not touched.
template <typename T>
__global__ void __launch_bounds__(128) mla_combine_kernel(const MlaKParams p, int head_dim) {
  const int64_t row = blockIdx.x;
  const int token = (int)(row / p.n_heads), head = (int)(row % p.n_heads);
  if (token >= p.q_cu[p.batch]) return;
  const float* ml = p.ml_part + row * p.n_splits * 2;
  float M = ATTN_M_INIT;
  for (int s = 0; s < p.n_splits; ++s) M = fmaxf(M, ml[2 * s]);
  const int d = 4 * threadIdx.x;
  if (d >= head_dim) return;
  const float* op = p.o_part + row * p.n_splits * (int64_t)head_dim + d;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
  for (int s = 0; s < p.n_splits; ++s) {
    const float ls = ml[2 * s + 1];
    if (ls > 0.f) {   // (a split without KV tokens: l = 0, nothing to add)
      const float w = fast_exp2(ml[2 * s] - M);
      l += ls * w;
      acc += *reinterpret_cast<const f32x4*>(op + (int64_t)s * head_dim) * w;
    }
  }
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  u32x2 o2;
  o2.x = pack2<T>(acc.x * inv, acc.y * inv);
  o2.y = pack2<T>(acc.z * inv, acc.w * inv);
  *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(p.out) + 2 * ((int64_t)token * p.o_ts + (int64_t)head * p.o_hs + d)) = o2;
}

// cache[slot_ids[t], :] = row[t, :] for the latent and the RoPE key, 16 bytes per lane
__global__ void __launch_bounds__(128) mla_set_kv_cache_kernel(const int* __restrict__ slot_ids, const char* __restrict__ kv,
                                                               const char* __restrict__ k_rope, int64_t kv_ts_b, int64_t kr_ts_b,
                                                               char* __restrict__ kv_cache, char* __restrict__ k_rope_cache,
                                                               int64_t kv_ss_b, int64_t kr_ss_b, int kv_chunks, int kr_chunks) {
  const int64_t t = blockIdx.x;
  const int64_t slot = slot_ids[t];
  if (slot < 0) return;  // a padding row (workgroup-uniform): nothing to append
  for (int c = threadIdx.x; c < kv_chunks + kr_chunks; c += blockDim.x) {
    if (c < kv_chunks)
      *reinterpret_cast<u32x4*>(kv_cache + slot * kv_ss_b + 16 * c) = *reinterpret_cast<const u32x4*>(kv + t * kv_ts_b + 16 * c);
    else
      *reinterpret_cast<u32x4*>(k_rope_cache + slot * kr_ss_b + 16 * (c - kv_chunks)) =
          *reinterpret_cast<const u32x4*>(k_rope + t * kr_ts_b + 16 * (c - kv_chunks));
  }
}

constexpr int MLA_TARGET_WGS = 256;      // one workgroup per CU
constexpr int MLA_MIN_SPLIT_KV = 256;    // KV tokens a split should at least own (8 tiles)
constexpr int MLA_MAX_SPLITS = 64;

bool mla_shape_supported(const slm_mla_args* a) {
  return (a->head_dim == 128 || a->head_dim == 256 || a->head_dim == 512) && a->rope_head_dim == MLA_ROPE &&
         (a->dtype == SLM_F16 || a->dtype == SLM_BF16);
}
// 32-row query blocks per workgroup: two once some sequence may have more than 32 rows
int mla_nq(const slm_mla_args* a) { return (int64_t)a->max_q_len * a->n_heads > 32 ? 2 : 1; }
int64_t mla_tiles_per_seq(const slm_mla_args* a) {
  const int64_t rows = (int64_t)a->max_q_len * a->n_heads, per = 32 * mla_nq(a);
  return (rows + per - 1) / per;
}
int mla_auto_splits(const slm_mla_args* a) {
  const int64_t wgs = mla_tiles_per_seq(a) * a->batch_size;
  if (wgs <= 0 || wgs >= MLA_TARGET_WGS) return 1;
  int64_t s = (MLA_TARGET_WGS + wgs - 1) / wgs;
  const int64_t by_len = a->max_kv_len / MLA_MIN_SPLIT_KV;
  if (s > by_len) s = by_len;
  if (s > MLA_MAX_SPLITS) s = MLA_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}
int mla_splits(const slm_mla_args* a) { return a->num_splits > 0 ? a->num_splits : mla_auto_splits(a); }
size_t mla_workspace_bytes(const slm_mla_args* a, int splits) {
  if (splits <= 1) return 0;
  return (size_t)a->n_tokens * (size_t)a->n_heads * (size_t)splits * (size_t)(a->head_dim + 2) * sizeof(float);
}
bool mla_sizes_ok(const slm_mla_args* a) {
  return a->batch_size >= 0 && a->n_tokens >= 0 && a->n_heads >= 1 && a->max_q_len >= 1 && a->max_kv_len >= 0 &&
         a->num_splits >= 0 && a->num_splits <= 1024;
}
bool stride16(int64_t elems) { return (elems * 2) % 16 == 0; }

template <typename T>
int mla_launch(const MlaKParams& kp, const slm_mla_args* a, int nq, hipStream_t st) {
  const int64_t grid = (int64_t)kp.tiles_per_seq * kp.batch * kp.n_splits;
  if (grid <= 0 || grid > 0x7fffffffLL) return SLM_ERR_UNSUPPORTED;
  const dim3 g((unsigned)grid), blk(64 * MLA_WAVES);
#define SLM_MLA(HDD)                                                                \
  do {                                                                              \
    if (nq == 2) hipLaunchKernelGGL((mla_kernel<T, HDD, 2>), g, blk, 0, st, kp);    \
    else hipLaunchKernelGGL((mla_kernel<T, HDD, 1>), g, blk, 0, st, kp);            \
  } while (0)
  if (a->head_dim == 512) SLM_MLA(512);
  else if (a->head_dim == 256) SLM_MLA(256);
  else SLM_MLA(128);
#undef SLM_MLA
  int rc = hip_check_launch();
  if (rc != SLM_OK || kp.n_splits <= 1) return rc;
  const int64_t rows = (int64_t)a->n_tokens * a->n_heads;
  if (rows > 0x7fffffffLL) return SLM_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((mla_combine_kernel<T>), dim3((unsigned)rows), dim3(128), 0, st, kp, (int)a->head_dim);
  return hip_check_launch();
}

}  // namespace

}  // namespace slm

using namespace slm;

extern "C" SLM_API size_t slm_mla_paged_kv_workspace_bytes(const slm_mla_args* a) {
  if (!a || !mla_sizes_ok(a) || a->head_dim <= 0) return 0;
  return mla_workspace_bytes(a, mla_splits(a));
}

extern "C" SLM_API int32_t slm_mla_paged_kv_auto_splits(const slm_mla_args* a) {
  if (!a || !mla_sizes_ok(a)) return 1;
  return mla_auto_splits(a);
}

extern "C" SLM_API int slm_mla_paged_kv(const slm_mla_args* a, void* stream) {
  if (!a) return SLM_ERR_INVALID_ARG;
  if (!mla_sizes_ok(a)) return SLM_ERR_INVALID_ARG;
  if (a->batch_size == 0 || a->n_tokens == 0) return SLM_OK;
  if (!a->out || !a->q || !a->q_rope || !a->kv_cache || !a->k_rope_cache || !a->q_cu_lens || !a->kv_cu_lens ||
      !a->block_table || !a->block_cu_lens)
    return SLM_ERR_INVALID_ARG;
  if (a->block_size <= 0 || !is_pow2(a->block_size)) return SLM_ERR_INVALID_ARG;
  if (!mla_shape_supported(a)) return SLM_ERR_UNSUPPORTED;
  if (!aligned16(a->out) || !aligned16(a->q) || !aligned16(a->q_rope) || !aligned16(a->kv_cache) ||
      !aligned16(a->k_rope_cache) || !stride16(a->o_stride[0]) || !stride16(a->o_stride[1]) ||
      !stride16(a->q_stride[0]) || !stride16(a->q_stride[1]) || !stride16(a->q_rope_stride[0]) ||
      !stride16(a->q_rope_stride[1]) || !stride16(a->kv_stride) || !stride16(a->k_rope_stride))
    return SLM_ERR_ALIGNMENT;
  const int splits = mla_splits(a);
  const size_t need = mla_workspace_bytes(a, splits);
  if (need > 0) {
    if (!a->workspace || a->workspace_bytes < need) return SLM_ERR_WORKSPACE;
    if (!aligned16(a->workspace)) return SLM_ERR_ALIGNMENT;
  }
  MlaKParams kp;
  kp.out = a->out; kp.q = a->q; kp.q_rope = a->q_rope; kp.kvc = a->kv_cache; kp.krc = a->k_rope_cache;
  kp.o_ts = a->o_stride[0]; kp.o_hs = a->o_stride[1];
  kp.q_ts = a->q_stride[0]; kp.q_hs = a->q_stride[1];
  kp.qr_ts = a->q_rope_stride[0]; kp.qr_hs = a->q_rope_stride[1];
  kp.kv_ss = a->kv_stride; kp.kr_ss = a->k_rope_stride;
  kp.q_cu = a->q_cu_lens; kp.kv_cu = a->kv_cu_lens; kp.bt = a->block_table; kp.bcu = a->block_cu_lens;
  kp.o_part = reinterpret_cast<float*>(a->workspace);
  kp.ml_part = need > 0 ? kp.o_part + (size_t)a->n_tokens * a->n_heads * splits * a->head_dim : nullptr;
  kp.batch = a->batch_size; kp.n_heads = a->n_heads;
  kp.block_shift = ilog2(a->block_size); kp.block_mask = a->block_size - 1;
  kp.n_splits = splits; kp.tiles_per_seq = (int)mla_tiles_per_seq(a);
  kp.scale_log2 = a->sm_scale * LOG2E;
  hip_clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return a->dtype == SLM_BF16 ? mla_launch<bf16_tag>(kp, a, mla_nq(a), st) : mla_launch<f16_tag>(kp, a, mla_nq(a), st);
}

extern "C" SLM_API int slm_mla_set_kv_cache(const int32_t* slot_ids, const void* kv, const void* k_rope,
                                            int64_t kv_token_stride, int64_t k_rope_token_stride, void* kv_cache,
                                            void* k_rope_cache, int64_t kv_slot_stride, int64_t k_rope_slot_stride,
                                            int64_t n_tokens, int32_t head_dim, int32_t rope_head_dim, int32_t dtype,
                                            void* stream) {
  if (n_tokens == 0) return SLM_OK;
  if (!slot_ids || !kv || !k_rope || !kv_cache || !k_rope_cache) return SLM_ERR_INVALID_ARG;
  if (n_tokens < 0 || n_tokens > 0x7fffffffLL || head_dim <= 0 || rope_head_dim <= 0) return SLM_ERR_INVALID_ARG;
  if (dtype != SLM_F16 && dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (head_dim % 8 != 0 || rope_head_dim % 8 != 0) return SLM_ERR_UNSUPPORTED;
  if (!aligned16(kv) || !aligned16(k_rope) || !aligned16(kv_cache) || !aligned16(k_rope_cache) ||
      !stride16(kv_token_stride) || !stride16(k_rope_token_stride) || !stride16(kv_slot_stride) ||
      !stride16(k_rope_slot_stride))
    return SLM_ERR_ALIGNMENT;
  hip_clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mla_set_kv_cache_kernel, dim3((unsigned)n_tokens), dim3(128), 0, st, slot_ids, (const char*)kv,
                     (const char*)k_rope, 2 * kv_token_stride, 2 * k_rope_token_stride, (char*)kv_cache,
                     (char*)k_rope_cache, 2 * kv_slot_stride, 2 * k_rope_slot_stride, head_dim / 8, rope_head_dim / 8);
  return hip_check_launch();
}
