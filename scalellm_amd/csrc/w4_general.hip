// w4_general.hip -- the GENERAL int4 GEMM kernel of slm_w4a16_gemm: 32 / 64 / 128-row tiles, one role per wave.
// Takes what no specialised kernel does (w4_plan.hip: narrow layers at 32 < M <= 128 and at M > 128, small M
// where the streams step aside); layout and dequant are described at the top of w4.hip.
#include "w4_plan.h"
#include "w4_epilogue.h"

namespace slm {

// W4_KC = 128: K chunk (LDS row = 256 B = 16 x 16-B slots, XOR-swizzled by row&15)

// MT : 32-token tiles per workgroup (BM = 32*MT)
// NTW: 32-column tiles per wave      (BN = 128*NTW, 4 waves split N: weights stay wave-private)
// NG : scale groups per 128-deep chunk (1 for group >= 128, 2 for 64, 4 for 32)
// PC : K chunks staged per pass; PC*MT*8 KiB per LDS buffer (32 KiB when PC*MT = 4), 2 buffers.
//
// Pipeline per pass (PC chunks = 2*PC weight loads per n-tile per lane):
//   top   : issue the NEXT pass's scale loads and A-tile loads (global -> registers)
//   body  : for every half-chunk (one 16-B weight load = 4 MFMA k-steps):
//             dequantise its 4 words -> 4 B fragments, re-issue that ring slot with the next pass's
//             load (pinned by sched_barrier so hipcc keeps COUNTED vmcnt waits), then the MFMAs,
//             A fragments coming from the swizzled LDS tile
//   bottom: the A registers (older in the vmcnt queue than the re-issued weight loads, so a counted
//           wait leaves a full pass of weight loads in flight) -> other LDS buffer, one barrier.
template <typename T, int MT, int NTW, int NG, int PC, bool POST>
__global__ void __launch_bounds__(256, (POST && PC * MT == 4 && MT < 4) ? 1 : 2) w4a16_gemm_kernel(const GemmKParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef typename Mfma<T>::frag frag_t;
  constexpr int BM = 32 * MT;
  constexpr int A_LD = PC * MT * 2;  // 16-B slots staged per thread per pass
  constexpr int CHUNK_BYTES = BM * 256;
  constexpr int BUF_BYTES = PC * CHUNK_BYTES;
  constexpr int HC = 2 * PC;  // half-chunks (16-B weight loads per lane) per pass
  // POST: per-(chunk, group, row) activation sums X, fp32, after the two A buffers
  constexpr int XS_FLOATS = PC * NG * BM;
  float* xs_base = reinterpret_cast<float*>(smem + 2 * BUF_BYTES);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bid = blockIdx.x;
  const int nb = bid % p.n_nblocks;
  bid /= p.n_nblocks;
  const int mb = bid % p.n_mblocks;
  const int ks = bid / p.n_mblocks;

  const int64_t m0 = (int64_t)mb * BM;
  const int c0 = ks * p.chunks_per_split;
  const int c1 = min(p.n_chunks, c0 + p.chunks_per_split);
  const int n_pass = (c1 - c0) / PC;  // host guarantees (c1 - c0) % PC == 0

  // this wave's column tiles (clamped: out-of-range tiles compute on the last valid tile, no store)
  const int64_t n_tiles = p.N / 32;
  int64_t ntile[NTW];
  bool nvalid[NTW];
#pragma unroll
  for (int t = 0; t < NTW; ++t) {
    const int64_t g = ((int64_t)nb * 4 + wave) * NTW + t;
    nvalid[t] = g < n_tiles;
    ntile[t] = nvalid[t] ? g : n_tiles - 1;
  }

  f32x16 acc[NTW][MT];
#pragma unroll
  for (int t = 0; t < NTW; ++t)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][m][r] = 0.f;

  f32x16 tmp[POST ? NTW : 1][POST ? MT : 1];  // per-group partial sums (POST form only)
  (void)tmp;

  // ---- A staging: thread -> (chunk, row, slot), global 16-B loads, swizzled LDS writes ----
  const char* abase = reinterpret_cast<const char*>(p.a);
  u32x4 areg[A_LD];
  auto a_load = [&](int cfirst) {  // chunks cfirst .. cfirst+PC-1
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
      const int idx = tid + 256 * i;
      const int ch = idx / (BM * 16), rem = idx % (BM * 16);
      const int row = rem >> 4, slot = rem & 15;
      const int64_t m = m0 + row;
      const int64_t mc = m < p.M ? m : p.M - 1;  // clamp (rows >= M are never stored)
      areg[i] = *reinterpret_cast<const u32x4*>(
          abase + 2 * (mc * p.lda + (int64_t)(cfirst + ch) * W4_KC + slot * 8));
    }
  };
  auto a_store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
      const int idx = tid + 256 * i;
      const int ch = idx / (BM * 16), rem = idx % (BM * 16);
      const int row = rem >> 4, slot = rem & 15;
      *reinterpret_cast<u32x4*>(smem + buf * BUF_BYTES + ch * CHUNK_BYTES + row * 256 +
                                ((slot ^ (row & 15)) << 4)) = areg[i];
      if constexpr (POST) {
        // the 16 slots of one (chunk, row) sit in 16 consecutive lanes (one DPP row): reduce the
        // 8-element partial sums over the 16/NG lanes of each scale group
        const u32x4 a = areg[i];
        float sum = lo_f32<T>(a.x) + hi_f32<T>(a.x) + lo_f32<T>(a.y) + hi_f32<T>(a.y) +
                    lo_f32<T>(a.z) + hi_f32<T>(a.z) + lo_f32<T>(a.w) + hi_f32<T>(a.w);
        sum = group_sum<16 / NG>(sum);
        if ((slot & (16 / NG - 1)) == 0)
          xs_base[buf * XS_FLOATS + (ch * NG + slot / (16 / NG)) * BM + row] = sum;
      }
    }
  };

  // ---- weight ring (one 16-B load per half-chunk per n-tile) and per-chunk scale/zero words ----
  u32x4 wreg[NTW][HC];
  uint32_t szcur[NTW][PC][NG], sznext[NTW][PC][NG];
  auto w_issue = [&](int t, int h, int cfirst) {  // half-chunk h of the pass starting at cfirst
    const uint32_t* wp = p.wq + ((((int64_t)cfirst * 2 + h) * n_tiles + ntile[t]) * 64 + lane) * 4;
    // plain (cacheable) loads, not non-temporal ones (round 4): a layer's weights are re-read within
    // ~0.4 ms -- by the second BM = 64 row block at M = 65...128 and by the second lane of the two-lane
    // decode step -- and a cacheable line is still in the Infinity Cache then.  Two-lane bs 256 step
    // 24.85 -> 23.98 ms, one lane 26.1 -> 25.9; stand-alone with rotating weights 3-6 % slower (124 ->
    // 132 us per layer at M = 128): the step is what counts.  The kernels that read every weight once
    // per launch (w4_ks / w4_gemv: M <= 32; w4_ws at M = 256) keep their nt loads.
    wreg[t][h] = *reinterpret_cast<const u32x4*>(wp);
  };
  auto sz_load = [&](uint32_t (&dst)[NTW][PC][NG], int cfirst) {
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
      for (int c = 0; c < PC; ++c)
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const int64_t grp = ((int64_t)(cfirst + c) * W4_KC + g * (W4_KC / NG)) >> p.gs_shift;
          dst[t][c][g] = p.sz[grp * p.N + ntile[t] * 32 + (lane & 31)];
        }
  };

  // dequantise (PRE) / unpack (POST) one 16-B weight vector into 4 MFMA B fragments
  auto make_frags = [&](const u32x4 wv, const uint32_t (&szc)[NG], int half, frag_t (&out)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int w8 = half * 4 + j;  // word index inside the 128-deep chunk
      uint32_t o[4];
      const uint32_t word = j == 0 ? wv.x : j == 1 ? wv.y : j == 2 ? wv.z : wv.w;
      if constexpr (POST) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = ((word >> (4 * i)) & 0x000F000Fu) | W4Magic<T>::bits;
      } else {
        const W4Dq<T> dq(szc[w8 * NG / 8]);
        dq.word(word, o);
      }
      const u32x4 packed = {o[0], o[1], o[2], o[3]};
      out[j] = __builtin_bit_cast(frag_t, packed);
    }
  };

  // Software pipeline inside the wave: while the MFMAs of half-chunk h run (matrix pipe), the VALU
  // dequantises half-chunk h+1 into the other fragment buffer; the ring slot of h+1 is then
  // re-issued one pass ahead (pinned by sched_barrier so the vmcnt waits stay counted).
  frag_t bfrag[2][NTW][4];
  if (n_pass > 0) {
    sz_load(szcur, c0);
    a_load(c0);
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
      for (int h = 0; h < HC; ++h) w_issue(t, h, c0);
    a_store(0);
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
      make_frags(wreg[t][0], szcur[t][0], 0, bfrag[0][t]);
      w_issue(t, 0, c0 + min(1, n_pass - 1) * PC);
    }
  }
  __syncthreads();

  const int mrow = lane & 31, kh = lane >> 5;
  for (int ps = 0; ps < n_pass; ++ps) {
    const int buf = ps & 1;
    const int cnext = c0 + min(ps + 1, n_pass - 1) * PC;   // clamped: last pass reloads itself
    const int cnext2 = c0 + min(ps + 2, n_pass - 1) * PC;
    sz_load(sznext, cnext);
    a_load(cnext);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int h = 0; h < HC; ++h) {
      const int cl = h >> 1;  // chunk within the pass
      const int cur = h & 1, nxt = cur ^ 1;
      const int hf = (h + 1) % HC;          // following half-chunk (first of the next pass at the end)
      const bool wrap = (h + 1) == HC;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int w8 = (h & 1) * 4 + j;
        const int slot = w8 * 2 + kh;
        constexpr int WPG = 8 / NG;  // k-steps (words) per scale group
        const bool g_first = (w8 % WPG) == 0, g_last = (w8 % WPG) == WPG - 1;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int row = m * 32 + mrow;
          const u32x4 av = *reinterpret_cast<const u32x4*>(
              smem + buf * BUF_BYTES + cl * CHUNK_BYTES + row * 256 + ((slot ^ (row & 15)) << 4));
          const frag_t af = __builtin_bit_cast(frag_t, av);
#pragma unroll
          for (int t = 0; t < NTW; ++t) {
            if constexpr (POST) {
              if (g_first) {
                f32x16 z;
#pragma unroll
                for (int r = 0; r < 16; ++r) z[r] = 0.f;
                tmp[t][m] = Mfma<T>::run(af, bfrag[cur][t][j], z);
              } else {
                tmp[t][m] = Mfma<T>::run(af, bfrag[cur][t][j], tmp[t][m]);
              }
              if (g_last) {
                // acc += s * (tmp - (magic + z) * X[row]) for this lane's column
                float sc, zm;
                W4Magic<T>::decode(szcur[t][cl][w8 * NG / 8], sc, zm);
                const float nzs = -zm * sc;
                const float* xs = xs_base + buf * XS_FLOATS + (cl * NG + w8 * NG / 8) * BM + m * 32 + 4 * kh;
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                  const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + 8 * q4);
#pragma unroll
                  for (int e = 0; e < 4; ++e) {
                    const int r = q4 * 4 + e;
                    acc[t][m][r] = fmaf(sc, tmp[t][m][r], fmaf(nzs, xv[e], acc[t][m][r]));
                  }
                }
              }
            } else {
              acc[t][m] = Mfma<T>::run(af, bfrag[cur][t][j], acc[t][m]);
            }
          }
        }
        // one word of the following half-chunk per k-step, in the shadow of the MFMAs above
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
          const u32x4 wv = wreg[t][hf];
          const int w8n = (hf & 1) * 4 + j;
          uint32_t o[4];
          const uint32_t word = j == 0 ? wv.x : j == 1 ? wv.y : j == 2 ? wv.z : wv.w;
          if constexpr (POST) {
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = ((word >> (4 * i)) & 0x000F000Fu) | W4Magic<T>::bits;
          } else {
            const uint32_t szw = wrap ? sznext[t][0][w8n * NG / 8] : szcur[t][hf >> 1][w8n * NG / 8];
            const W4Dq<T> dq(szw);
            dq.word(word, o);
          }
          const u32x4 packed = {o[0], o[1], o[2], o[3]};
          bfrag[nxt][t][j] = __builtin_bit_cast(frag_t, packed);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < NTW; ++t) w_issue(t, hf, wrap ? cnext2 : cnext);  // slot hf is free again
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
      for (int c = 0; c < PC; ++c)
#pragma unroll
        for (int g = 0; g < NG; ++g) szcur[t][c][g] = sznext[t][c][g];
    a_store(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue (C/D layout: w4_epilogue.h)
  const DenseRows rows{m0, p.M};
  if (p.silu && p.split_k == 1) {
    // SLM_W4_SILU_MUL: column tiles are (gate, up) pairs.  NTW == 2: both tiles of a pair are this
    // wave's own; NTW == 1: waves (0, 1) and (2, 3) hold a pair, exchanged through the (now idle) A buffers
    if constexpr (NTW == 1) {
      uint16_t* ex = reinterpret_cast<uint16_t*>(smem) + (wave >> 1) * (MT * 1024);
      cd_silu_exchange<T, MT>(acc[0], rows, lane, ex, wave & 1, !(wave & 1) && nvalid[0], p.bias, ntile[0], p.c, p.ldc,
                              ntile[0] >> 1);
    } else {
      if (!nvalid[0]) return;
      const int64_t gcol = ntile[0] * 32 + (lane & 31);
      const float bg = cd_bias<T>(p.bias, gcol), bu = cd_bias<T>(p.bias, gcol + 32);
      cd_store_silu<T, MT>(
          acc[0], bg, [&](int m, int r) { return lo_f32<T>((uint32_t)pack1<T>(acc[1][m][r] + bu)); }, rows, lane, p.c,
          p.ldc, (ntile[0] >> 1) * 32 + (lane & 31));
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < NTW; ++t) {
    if (!nvalid[t]) continue;
    const int64_t n = ntile[t] * 32 + (lane & 31);
    float bv = 0.f;
    if (p.split_k == 1 && p.bias) {
      const uint16_t braw = reinterpret_cast<const uint16_t*>(p.bias)[n];
      bv = lo_f32<T>((uint32_t)braw);
    }
    cd_store_splitk<T, MT>(acc[t], rows, lane, p.split_k == 1, p.c, p.ldc, ntile[t], bv, p.part, (int64_t)ks * p.M, p.N);
  }
}

template <typename T, int MT, int NTW, int PC>
static void launch_gemm_ng(const GemmKParams& kp, const GemmPlan& pl, hipStream_t st) {
  const dim3 grid((unsigned)pl.n_blocks()), blk(256);
#define SLM_GEMM(NGG, POSTT)                                                                        \
  hipLaunchKernelGGL((w4a16_gemm_kernel<T, MT, NTW, NGG, PC, POSTT>), grid, blk, pl.lds_bytes, st, kp)
  if (pl.general.post) {  // (the plan only sets it where w4_post_fits: the other instantiations are not built)
    switch (pl.ng) {
      case 4: if constexpr (w4_post_fits(MT, NTW, 4, PC)) SLM_GEMM(4, true); break;
      case 2: if constexpr (w4_post_fits(MT, NTW, 2, PC)) SLM_GEMM(2, true); break;
      default: if constexpr (w4_post_fits(MT, NTW, 1, PC)) SLM_GEMM(1, true); break;
    }
    return;
  }
  switch (pl.ng) {
    case 4: if constexpr (w4_pre_fits(MT, NTW, 4, PC)) SLM_GEMM(4, false); break;
    case 2: SLM_GEMM(2, false); break;
    default: SLM_GEMM(1, false); break;
  }
#undef SLM_GEMM
}

template <typename T, int MT, int NTW>
static void launch_gemm_pc(const GemmKParams& kp, const GemmPlan& pl, hipStream_t st) {
  constexpr int PCMAX = 4 / MT;
  if (pl.general.pc == PCMAX) launch_gemm_ng<T, MT, NTW, PCMAX>(kp, pl, st);
  else if constexpr (PCMAX >= 4) {
    if (pl.general.pc == 2) launch_gemm_ng<T, MT, NTW, 2>(kp, pl, st);
    else launch_gemm_ng<T, MT, NTW, 1>(kp, pl, st);
  } else launch_gemm_ng<T, MT, NTW, 1>(kp, pl, st);
}

template <typename T>
static void launch_gemm(const GemmKParams& kp, const GemmPlan& pl, hipStream_t st) {
  if (pl.general.mt == 4) launch_gemm_pc<T, 4, 1>(kp, pl, st);
  else if (pl.general.mt == 2 && pl.general.ntw == 2) launch_gemm_pc<T, 2, 2>(kp, pl, st);
  else if (pl.general.mt == 2) launch_gemm_pc<T, 2, 1>(kp, pl, st);
  else if (pl.general.ntw == 2) launch_gemm_pc<T, 1, 2>(kp, pl, st);
  else launch_gemm_pc<T, 1, 1>(kp, pl, st);
}

void launch_gemm_general(const GemmKParams& kp, int dtype, const GemmPlan& pl, hipStream_t st) {
  dispatch_dtype(dtype, [&](auto t) { launch_gemm<decltype(t)>(kp, pl, st); });
}

}  // namespace slm
