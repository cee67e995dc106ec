// w4_plan.hip -- the planner of slm_w4a16_gemm: validate the call, summarise its shape, then ask one
// planner per kernel, in precedence order, whether it takes the call (plan_gemm at the bottom).  Host code
// only: a pure function of the argument block and the tuning table, no HIP call.  What a kernel CAN run is
// its own file's business (gemv_supported, gemv_global_splits, gemm_ks_config_ok, w4_post_fits,
// w4_pre_fits); WHERE it runs is decided here, next to the measurements behind each boundary.
// tests/test_w4_plan_cpu.py pins every field of the result over tests/golden/w4_plan_table.npz;
// slm_w4a16_gemm_plan (include/slm_hip.h) shows it to callers.
#include "w4_plan.h"
#include "tuning.h"

namespace slm {

static int validate(const slm_w4_gemm_args* a) {
  if (!a) return SLM_ERR_INVALID_ARG;
  if (a->M < 0 || a->K <= 0 || a->N <= 0) return SLM_ERR_INVALID_ARG;
  if (a->dtype != SLM_F16 && a->dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (a->K % W4_KC || a->N % 32) return SLM_ERR_UNSUPPORTED;  // reference: K%128, N%64
  if (a->flags & ~(SLM_W4_DEFER_REDUCE | SLM_W4_SILU_MUL | SLM_W4_SHARES_CHIP)) return SLM_ERR_INVALID_ARG;
  if (a->flags & SLM_W4_SILU_MUL) {
    if (a->flags & SLM_W4_DEFER_REDUCE) return SLM_ERR_INVALID_ARG;
    if (a->N % 64) return SLM_ERR_UNSUPPORTED;
  }
  if (!w4_group_size_valid(a->group_size, a->K)) return SLM_ERR_UNSUPPORTED;
  return SLM_OK;
}

// what the planners ask about a (valid) call, computed once
struct Shape {
  int n_chunks;                     // K / 128
  int n_tiles;                      // N / 32
  int64_t tiles4, tiles8, tiles16;  // 128 x 128, 256 x 128 and 256 x 256 tiles that cover M x N
  bool silu;
  // 32-bit addressing of the kernels other than the general one
  bool tables_fit_u32;  // packed weights and scale table below 4 GiB
  bool a_fits_i31;      // byte offsets into A below 2 GiB
  bool c_fits_i31;      // byte offsets into C and into one fp32 slab below 2 GiB
};

static Shape shape_of(const slm_w4_gemm_args* a) {
  Shape s;
  s.n_chunks = (int)(a->K / W4_KC);
  s.n_tiles = (int)(a->N / 32);
  const int64_t n128 = (a->N + 127) / 128, m256 = (a->M + 255) / 256;
  s.tiles4 = ((a->M + 127) / 128) * n128;
  s.tiles8 = m256 * n128;
  s.tiles16 = m256 * ((a->N + 255) / 256);
  s.silu = (a->flags & SLM_W4_SILU_MUL) != 0;
  s.tables_fit_u32 = a->K * a->N / 2 < ((int64_t)1 << 32) && (a->K / a->group_size) * a->N * 4 < ((int64_t)1 << 32);
  s.a_fits_i31 = ((a->M - 1) * a->lda + a->K) * 2 < ((int64_t)1 << 31);
  s.c_fits_i31 = ((a->M - 1) * a->ldc + a->N) * 2 < ((int64_t)1 << 31) && a->M * a->N * 4 < ((int64_t)1 << 31);
  return s;
}

// M <= 4: dot2 GEMV (measured: the GEMV wins on every layer shape at M = 1 and loses on some at M = 2..4, so
// the default is M = 1 only; SLM_W4_GEMV=2 forces it for M <= 4; its 32-bit offsets need < 4 GiB tables)
static bool plan_gemv(const slm_w4_gemm_args* a, const Shape& s, GemmPlan* pl) {
  const int gemv_mode = tune_get(TUNE_W4_GEMV, 1);
  if (!(gemv_mode != 0 && (a->M == 1 || gemv_mode == 2) && gemv_supported(a->M, a->K, a->group_size) &&
        s.tables_fit_u32))
    return false;
  pl->kernel = W4Kernel::GEMV;
  // K is split inside the workgroup: no partials, no reduce launch.  Exception: when the caller
  // defers the reduction to the consumer anyway (SLM_W4_DEFER_REDUCE: RMSNorm, RoPE + append)
  // a narrow layer is ALSO split across workgroups so that its launch covers all the CUs --
  // o_proj at M = 1 has 128 column tiles = 128 workgroups on 256 CUs, and a CU's load path
  // (~14 B/clk) caps 128 of them at ~3.3 TB/s.
  pl->split_k = gemv_global_splits(a->M, a->K, a->N, (a->flags & SLM_W4_DEFER_REDUCE) && !a->bias && !a->perm);
  pl->chunks_per_split = s.n_chunks;
  pl->n_mblocks = 1;
  pl->n_nblocks = gemv_workgroups(a->K, a->N, s.silu);
  pl->lds_bytes = gemv_lds_bytes(a->M, a->K, false);
  return true;
}

// both need the 32-bit addressing; SLM_W4_SMALL = 0 sends M <= 32 to the general kernel's MT = 1 tiles
static bool lean_stream_ok(const slm_w4_gemm_args* a, const Shape& s) {
  return a->M <= 32 && tune_get(TUNE_W4_SMALL, 1) != 0 && s.tables_fit_u32 && s.a_fits_i31;
}

static void commit_ks(const Shape& s, int mt, int cw, int nw, int tpw, int ksplit, GemmPlan* pl) {
  // tiles per workgroup = about one workgroup per CU
  if (tpw <= 0) {
    tpw = (int)(((int64_t)ksplit * s.n_tiles + 128) / 256);
    if (tpw < 1) tpw = 1;
  }
  if (s.silu) tpw = (tpw + 1) & ~1;  // (gate, up) tile pairs stay in one workgroup
  if (tpw > s.n_tiles) tpw = s.n_tiles;
  pl->kernel = W4Kernel::KS;
  pl->ks = {mt, cw, nw, tpw};
  pl->split_k = ksplit;
  pl->chunks_per_split = nw * cw;
  pl->n_mblocks = 1;
  pl->n_nblocks = (s.n_tiles + tpw - 1) / tpw;
  pl->lds_bytes = w4_ks_lds_bytes(nw);
}

// M <= 32 (M == 1 stays on the GEMV): the K-sliced weight stream (w4_ks.hip) -- K split over the
// waves of a workgroup (activations in registers), partial tiles reduced through LDS.  Launch
// shape from tools/bench_small_gemm.py sweeps on MI355X (profiles/r03_ks_sweep_m32.jsonl): the
// widest K slice per wave wins on every layer shape (fewest workgroups re-reading the
// activations), tiles per workgroup = about one workgroup per CU.  The slice width depends on K
// only -- NOT on the epilogue flags -- so that a fused SiLU*mul call and the plain call sum in the
// same order (bit-identical results, tests/test_w4_silu_gpu.py).
static bool plan_ks_one_tile(const slm_w4_gemm_args* a, const Shape& s, GemmPlan* pl) {
  if (!(tune_get(TUNE_W4_KS, 1) != 0 && a->M >= 1 && lean_stream_ok(a, s) && s.c_fits_i31)) return false;
  const int cw_max = pl->ng == 4 ? 2 : 4;
  int nw = tune_get(TUNE_W4_KS_NW, 0), cw = tune_get(TUNE_W4_KS_CW, 0);
  const int forced_split = tune_get(TUNE_W4_SPLITK, 0);
  if (nw == 0 && cw == 0 && forced_split > 0) {  // tests / sweeps that pin the split: honour it or step aside
    for (int tw = 8; tw >= 4 && !nw; tw -= 4)
      for (int tc = cw_max; tc >= 1 && !nw; tc >>= 1)
        if ((s.n_chunks + tw * tc - 1) / (tw * tc) == forced_split && gemm_ks_config_ok(pl->ng, tc, tw, 1)) {
          nw = tw;
          cw = tc;
        }
  } else {
    if (nw == 0) nw = s.n_chunks <= 4 ? 4 : 8;
    if (cw == 0) {
      cw = 1;
      while (cw < cw_max && nw * cw < s.n_chunks) cw *= 2;
    }
  }
  if (!(nw && cw && gemm_ks_config_ok(pl->ng, cw, nw, 1))) return false;
  const int ksplit = (s.n_chunks + nw * cw - 1) / (nw * cw);
  if (!(ksplit <= 16 && (forced_split <= 0 || ksplit == forced_split))) return false;
  commit_ks(s, 1, cw, nw, tune_get(TUNE_W4_KS_TPW, 0), ksplit, pl);
  return true;
}

// 33 <= M <= 64 (round 4; the default outside the two-lane steps since round 6): the K-sliced stream with TWO row tiles -- every
// weight word unpacked once for two MFMAs.  One chunk of K per wave (the activations of both row
// tiles fill the registers), 8 waves: a workgroup covers 1024 of K, the rest is split across
// workgroups (fp32 slabs, summed by the consumer under SLM_W4_DEFER_REDUCE or by the reduce kernel).
// Measured (profiles/r04_ks_mt2.jsonl, M = 64 stand-alone): qkv 19.5 -> 17.6 us, gate_up 40.4 -> 36.6,
// o 15.8 -> 15.6, down 26.3 -> 36.1 (14 slabs: excluded below); the bs = 64 decode step 9.07 -> 8.93 ms.
// NOT under the two-lane decode step (decode.py; SLM_W4_SHARES_CHIP): there its 512-thread, 236-VGPR workgroups
// cannot share a CU with the other lane's attention waves and wait for them instead -- bs = 128
// (two lanes of 64 rows) 14.2 -> 21.5 ms -- and the stand-alone gain is small because A (512 KB at
// M = 64, K = 4096) cannot stay on one CU: either K is split over CUs (slab traffic, this kernel) or
// A is re-streamed per column tile (the general kernel); the step from M = 32 stays.
// Round 6: ON by default where the caller does not say the call shares the chip (SLM_W4_SHARES_CHIP, set by
// the two-lane decode steps): M = 33 / 48 / 64 layer chain 96 / 97 / 101 -> 89 / 90 / 93 us, bs = 64 step
// 9.17 -> 8.95 ms (profiles/r06_ks_mt2_default.jsonl).  SLM_W4_KS_MT2 = 0 never, 1 / 2 always (2: any split).
static bool plan_ks_two_tiles(const slm_w4_gemm_args* a, const Shape& s, GemmPlan* pl) {
  const int mt2_knob = tune_get(TUNE_W4_KS_MT2, -1);
  const bool mt2_on = mt2_knob > 0 || (mt2_knob < 0 && !(a->flags & SLM_W4_SHARES_CHIP));
  if (!(tune_get(TUNE_W4_KS, 1) != 0 && mt2_on && a->M > 32 && a->M <= 64 && s.tables_fit_u32 && s.a_fits_i31 &&
        s.c_fits_i31 && gemm_ks_config_ok(pl->ng, 1, 8, 2)))
    return false;
  const int ksplit = (s.n_chunks + 7) / 8;
  const int forced_split = tune_get(TUNE_W4_SPLITK, 0);
  // deep K (down_proj: 14 slabs of fp32 partials) loses to the general kernel's 8-way split with
  // wider tiles (M = 64: 36.1 vs 26.3 us); up to 4 slabs it wins or ties (qkv 17.6 vs 19.5, o 15.6 vs
  // 15.8, gate_up 36.6 vs 40.4 us; profiles/r04_ks_mt2.jsonl).  SLM_W4_KS_MT2=2 lifts the bound (tests).
  const int max_split = mt2_knob >= 2 ? 16 : 4;
  if (!(ksplit <= max_split && (forced_split <= 0 || ksplit == forced_split))) return false;
  commit_ks(s, 2, 1, 8, tune_get(TUNE_W4_KS_TPW, 0), ksplit, pl);
  return true;
}

// the tiled kernels: small (32 x 128), general (32 / 64 / 128 x 128 or 256), ws (256 x 128), xl (256 x 256)
// M > 128: 32-row tiles per workgroup among 2 / 4 (general), 8 (w4_ws.hip), 16 = the 256 x 256 tiles of
// w4_xl.hip (8 row tiles: the code 16 is what SLM_W4_MT calls them)
static int large_m_tile(const slm_w4_gemm_args* a, const Shape& s) {
  // the wave-specialised 256 x 128 kernel (w4_ws.hip) when its tiles alone keep about
  // half of the 256 CUs busy (measured: 0.89-1.06 PFLOP/s vs 0.74-0.86 for the single-role
  // kernel on gate_up/down at M = 256..2048); narrow layers stay on the 128 x 128 kernel, whose
  // 2 workgroups per CU need less split-K.  Its A addressing uses 32-bit offsets.
  int mt = (s.tiles8 >= 112 && s.a_fits_i31) ? 8 : ((s.tiles4 >= 256 || a->K >= 8192) ? 4 : 2);
  // prefill-sized problems: the symmetric 256 x 256 kernel (w4_xl.hip) when its tiles fill whole
  // rounds of the 256 CUs (measured +5..7 % over the 256 x 128 kernel there, -36 % when they don't)
  const int64_t rounds = (s.tiles16 + 255) / 256;
  if (s.a_fits_i31 && s.tiles16 >= 224 && s.tiles16 * 100 >= rounds * 256 * 87) mt = 16;
  // ... and when the 256 x 128 tiles need MORE rounds than they save (round 5, M = 2648 -- the mixed step's row
  // count: o 4096 x 4096 = 176 / 352 tiles: one 69 %-full round of 256 x 256 tiles 102.6 us against two rounds of
  // 256 x 128 tiles 117.4; down 340.8 against 382.8): a 256 x 128 tile takes 0.58 of a 256 x 256 tile's time
  // (profiles/r05_gemm_large_m.jsonl; layer chain 1282 -> 1192 us at M = 2648, 1400 -> 1322 at 3072,
  // the mixed step 55.1 -> 52.6 ms)
  const int64_t rounds8 = (s.tiles8 + 255) / 256;
  // (and only with its rounds >= 65 % full: at 56 % -- qkv at M = 1536, 144 tiles -- the layer chain LOSES 5.6 %)
  if (s.a_fits_i31 && mt == 8 && rounds8 >= 2 && rounds * 100 < rounds8 * 58 && s.tiles16 * 100 >= rounds * 256 * 65 &&
      tune_get(TUNE_W4_XL_MODEL, 1) != 0)
    mt = 16;
  return mt;
}

// Round 6: the STREAM-K form of the 256 x 256 kernel (w4_xl.hip): the tile x K work cut into 256 equal ranges
// -- no round of tiles is left part-filled.  Cost model in units of one 256 x 256 tile's time: the chosen
// kernel's rounds (a 256 x 128 tile: 0.58) against 1.4 x tiles16 / 256 (measured 1.28...1.41 over M = 1536...3072:
// a second pipeline fill per workgroup, the partial tiles' round trip, a fuller chip's lower clock;
// profiles/r06_gemm_streamk.jsonl).  At least half a tile per
// workgroup (a tile is then cut into at most three pieces); not with the SiLU pair epilogue (gate_up fills
// its rounds), not next to another stream (its workgroups wait for each other: SLM_W4_SHARES_CHIP), not
// under a forced tile or split (SLM_W4_MT, SLM_W4_SPLITK).
static bool stream_k_wins(const slm_w4_gemm_args* a, const Shape& s) {
  const int sk_mode = tune_get(TUNE_W4_XL_SK, 1);
  if (!(a->M > 128 && s.a_fits_i31 && sk_mode != 0 && s.tiles16 >= 128 && a->N % 256 == 0 &&
        !(a->flags & (SLM_W4_SILU_MUL | SLM_W4_SHARES_CHIP)) && !tune_is_set(TUNE_W4_MT) && !tune_is_set(TUNE_W4_SPLITK)))
    return false;
  const int mt = large_m_tile(a, s);
  const double cur = mt == 16 ? (double)((s.tiles16 + 255) / 256) : mt == 8 ? 0.58 * (double)((s.tiles8 + 255) / 256) : 1e30;
  const double sk = 1.40 * (double)s.tiles16 / 256.0;
  return sk_mode >= 2 || sk < 0.97 * cur;
}

// Row tile of a call the general / ws / xl kernels take.  Launch shape from tools/sweep_gemm.py on MI355X
// (profiles/r01_gemm_sweep.jsonl):
//  M <= 64 : one M tile (MT = 1/2), post-scaled dequant, ~256 workgroups (split-K fills the chip)
//  M  > 64 : BM = 128 when the N x M tiling alone gives >= 256 tiles or K is deep, else BM = 64;
//            ~512 workgroups (2 per CU), split-K <= 8
static int tile_rows(const slm_w4_gemm_args* a, const Shape& s) {
  int mt;
  if (a->M <= 32) mt = 1;
  else if (a->M <= 64) mt = 2;
  else if (a->M <= 128) {
    // BM = 128 when its tiles alone fill the chip, or when K is deep AND there are enough column
    // tiles to spread (a deep, very narrow shard -- 70B TP=8 qkv: 8192 x 1280 -- runs 20 % faster
    // on twice as many BM = 64 tiles: 22.0 -> 17.7 us)
    // (round 4: the deep-K rule starts at 64 tiles, not 32.  Llama-3-8B's down_proj -- 14336 x 4096, 32 tiles --
    // is 3 % faster alone on BM = 128 (33.0 vs 34.1 us at M = 128), but in the two-lane decode step its 64 KiB,
    // ~200-VGPR workgroups share a CU badly with the attention stream's: 79 -> 135 us per call once the stream
    // kernel keeps two row chunks per lane, 58 us on BM = 64 tiles like the other three layers)
    mt = (s.tiles4 >= 256 || (a->K >= 8192 && s.tiles4 >= 64)) ? 4 : 2;
  } else {
    // (a call the stream-K model wants but whose K the stream-K form cannot cut -- plan_xl_sk -- keeps the
    // 256 x 256 tiles)
    mt = stream_k_wins(a, s) ? 16 : large_m_tile(a, s);
  }
  mt = tune_get(TUNE_W4_MT, mt);
  if (a->M > 64 && a->M <= 128 && a->N >= 16384) mt = tune_get(TUNE_W4_MT_WIDE, mt);  // (wide layers: gate_up)
  // 8 = wave-specialised 256 x 128 kernel (w4_ws.hip), 16 = symmetric 256 x 256 kernel (w4_xl.hip)
  if (mt != 1 && mt != 2 && mt != 4 && mt != 8 && mt != 16) mt = 4;
  if (mt >= 8 && !s.a_fits_i31) mt = 4;
  return mt;
}

// grid and split-K of mt x ntw tiles; returns PC, the chunks the general kernel stages per pass
static int plan_tiles(const slm_w4_gemm_args* a, const Shape& s, int mt, int ntw, GemmPlan* pl) {
  const int bm = mt == 16 ? 256 : 32 * mt, bn = mt == 16 ? 256 : 128 * ntw;
  pl->n_mblocks = (int)((a->M + bm - 1) / bm);
  pl->n_nblocks = (int)((a->N + bn - 1) / bn);
  const int64_t tiles = (int64_t)pl->n_mblocks * pl->n_nblocks;
  // pass = PC chunks per LDS buffer (PC*MT <= 4); one chunk per pass measured best or equal
  int pc = tune_get(TUNE_W4_PC, 1);
  if (pc != 1 && pc != 2 && pc != 4) pc = 1;
  if (pc * mt > 4) pc = mt >= 4 ? 1 : 4 / mt;
  while (pc > 1 && s.n_chunks % pc) pc >>= 1;
  if (!w4_pre_fits(mt, ntw, pl->ng, pc)) pc = 1;  // (a knob combination that does not fit the registers)
  const int n_units = s.n_chunks / pc;  // split-K granularity = whole passes
  int split_k = tune_get(TUNE_W4_SPLITK, 0);
  if (split_k <= 0) {
    const int64_t target = (a->M <= 64 || mt >= 8) ? 256 : tune_get(TUNE_W4_SPLIT_TARGET, 512);
    int64_t want = (target + tiles / 2) / (tiles > 0 ? tiles : 1);
    // M > 64: keep >= 8 chunks (1024 of K) per split -- short K (row-parallel TP shards) does not
    // amortise the fp32 partial round trip
    const int64_t cap = a->M <= 64 ? 8 : (s.n_chunks / 8 > 0 ? s.n_chunks / 8 : 1);
    if (want > cap) want = cap;
    if (want > 8) want = 8;
    if (want < 1) want = 1;
    if (want > n_units) want = n_units;
    split_k = (int)want;
  }
  if (split_k > n_units) split_k = n_units;
  const int units_per_split = (n_units + split_k - 1) / split_k;
  pl->chunks_per_split = units_per_split * pc;
  pl->split_k = (n_units + units_per_split - 1) / units_per_split;
  return pc;
}

// M <= 32 where the K-sliced kernel steps aside (SLM_W4_KS = 0, a forced split it cannot realise, C past
// 2 GiB): the lean weight-streaming kernel (w4_small.hip)
static bool plan_small(const slm_w4_gemm_args* a, const Shape& s, GemmPlan* pl) {
  if (!lean_stream_ok(a, s)) return false;
  pl->kernel = W4Kernel::SMALL;
  plan_tiles(a, s, 1, 1, pl);
  pl->lds_bytes = W4_SMALL_LDS_BYTES;
  return true;
}

// 65 <= M <= 128 (round 5): all rows in ONE workgroup (w4_m128.hip) -- every weight word fetched and
// dequantised once for 4 MFMAs instead of once per 64-row block for 2 -- in 132-VGPR / 32-KiB workgroups
// that sit twice on a CU next to the decode attention stream of the other lane.  Split-K aims at two
// workgroups per CU with >= 512 of K each (the consumers take up to 16 slabs).
// Where (measured, profiles/r05_m128_*.jsonl): deep-K layers (K >= 8192: the Llama-3-70B shapes, where the
// general kernel already took its ~200-VGPR BM = 128 tiles) -- the 70B step 50.6 -> 49.4 ms.  On the
// Llama-3-8B shapes (K = 4096, and 14336 x 4096) it ties the BM = 64 general kernel alone and in the two-lane
// step: there the GEMMs are starved of HBM bandwidth by the attention stream, not bound by their
// instruction count (tools/probe_corun.py), and the plan with fewer, longer workgroups leaves the chain
// longer.  SLM_W4_M128 = 1 forces it everywhere (tests), 0 disables it; a forced SLM_W4_MT keeps the general kernel.
static bool plan_m128(const slm_w4_gemm_args* a, const Shape& s, GemmPlan* pl) {
  const int m128_mode = tune_get(TUNE_W4_M128, -1);
  // ... and wide enough to fill the chip with 128-column tiles (>= 64 of them): the TP = 8 shards of the 70B
  // layers (8192 x 1280, 8192 x 7168) stay on twice as many BM = 64 tiles (rank-0 shard step 11.97 vs 12.11 ms)
  const bool deep_wide = a->K >= 8192 && a->N >= 8192;
  if (!(m128_mode != 0 && (m128_mode > 0 || deep_wide) && a->M > 64 && a->M <= 128 && !tune_is_set(TUNE_W4_MT) &&
        s.tables_fit_u32 && s.a_fits_i31))
    return false;
  // 256-column workgroups (8 column tiles share the activation panel a CU ingests, w4_m128.hip "CT"): one
  // 512-thread workgroup per CU is the fill they aim at.  Default where the plan picks this kernel itself (the
  // deep, wide 70B shapes: layer at M = 128 306.6 -> 285.0 us, every GEMM of it faster,
  // profiles/r05_m128_ct8.jsonl); forced onto the 8B shapes (SLM_W4_M128 = 1) the two forms tie.
  const int ct = tune_get(TUNE_W4_M128_CT, deep_wide ? 8 : 4) == 8 ? 8 : 4;
  const int64_t tiles1 = (a->N + 32 * ct - 1) / (32 * ct);
  const int64_t target = tune_get(TUNE_W4_M128_SPLITS, ct == 8 ? 256 : 512);
  int64_t want = (target + tiles1 / 2) / tiles1;
  const int64_t cap = s.n_chunks / 4 > 0 ? s.n_chunks / 4 : 1;
  if (want > cap) want = cap;
  if (want > 16) want = 16;
  if (want < 1) want = 1;
  const int forced = tune_get(TUNE_W4_SPLITK, 0);
  if (forced > 0) want = forced < s.n_chunks ? forced : s.n_chunks;
  const int per = (int)((s.n_chunks + want - 1) / want);
  pl->kernel = W4Kernel::M128;
  pl->n_mblocks = 1;
  pl->n_nblocks = (int)tiles1;
  pl->chunks_per_split = per;
  pl->split_k = (s.n_chunks + per - 1) / per;
  // ring depth 4 where it was measured (Llama-3-70B shapes, profiles/r05_m128_70b_shapes.jsonl: layer 318 ->
  // 310 us, gate_up 155 -> 148, down 83 -> 82); the general kernel's BM = 64 tiles: 336 us
  int wd = tune_get(TUNE_W4_M128_WD, a->K >= 8192 ? 4 : 2);
  if (wd != 4 || (2 * per) % 4 != 0 || s.n_chunks % per != 0) wd = 2;
  // two waves per column tile (512-thread workgroups) up to two workgroups per CU: measured on the 70B shapes
  // (profiles/r05_m128_kw.jsonl, one box): layer 333 -> 313 us, gate_up 155 -> 148 (448 workgroups), the others
  // within 1 us (480 / 512 workgroups).  SLM_W4_M128_KW: 1 / 2 force a form.
  const int kw_knob = tune_get(TUNE_W4_M128_KW, 0);
  int kw = kw_knob == 2 || (kw_knob != 1 && (int64_t)pl->n_nblocks * pl->split_k <= 512) ? 2 : 1;
  if (ct == 8) kw = 1;
  // activations by LDS-DMA (256-column form): 70B layer at M = 128 284.6 -> 271.1 us (profiles/r05_m128_adma.jsonl)
  pl->m128 = {wd, kw, ct, ct == 8 && tune_get(TUNE_W4_M128_ADMA, 1) != 0};
  pl->lds_bytes = W4_M128_LDS_BYTES;
  return true;
}

// the stream-K form where its cost model wins (stream_k_wins) and K can be cut
static bool plan_xl_sk(const slm_w4_gemm_args* a, const Shape& s, GemmPlan* pl) {
  if (!stream_k_wins(a, s)) return false;
  // equal ranges of the work list, in whole 64-deep chunk QUADS (the kernel's ring granularity: 2 chunks of 128)
  int64_t per = (s.tiles16 * s.n_chunks + W4_XL_SK_WGS - 1) / W4_XL_SK_WGS;
  per = (per + 1) & ~(int64_t)1;
  if (!(per >= 2 && (s.n_chunks & 1) == 0 && per < ((int64_t)1 << 30))) return false;
  pl->kernel = W4Kernel::XL_SK;
  pl->xl_sk.sk_per = (int)per;
  pl->n_mblocks = (int)((a->M + 255) / 256);
  pl->n_nblocks = (int)((a->N + 255) / 256);
  pl->split_k = 1;
  pl->chunks_per_split = s.n_chunks;
  pl->lds_bytes = W4_XL_LDS_BYTES;
  return true;
}

// everything else: the tile kernels by row tile.  Never steps aside.
static bool plan_tiled(const slm_w4_gemm_args* a, const Shape& s, GemmPlan* pl) {
  const int mt = tile_rows(a, s);
  int ntw = tune_get(TUNE_W4_NTW, 1);
  if (ntw != 1 && ntw != 2) ntw = 1;
  if (mt >= 4) ntw = 1;
  const int pc = plan_tiles(a, s, mt, ntw, pl);
  if (mt >= 8) {
    pl->kernel = mt == 16 ? W4Kernel::XL : W4Kernel::WS;
    pl->lds_bytes = mt == 16 ? W4_XL_LDS_BYTES : W4_WS_LDS_BYTES;
    return true;
  }
  pl->kernel = W4Kernel::GENERAL;
  // small-M tiles use the post-scaled form (7 VALU per 8 weights instead of ~27)
  const int post = tune_get(TUNE_W4_POST, a->M <= 64 ? 1 : 0) != 0 && w4_post_fits(mt, ntw, pl->ng, pc);
  pl->general = {mt, ntw, pc, post};
  pl->lds_bytes = (size_t)2 * pc * 32 * mt * 256 + (post ? (size_t)2 * pc * pl->ng * 32 * mt * sizeof(float) : 0);
  return true;
}

int plan_gemm(const slm_w4_gemm_args* a, GemmPlan* pl) {
  const int rc = validate(a);
  if (rc != SLM_OK) return rc;
  const Shape s = shape_of(a);
  *pl = GemmPlan{};
  pl->ng = a->group_size == 32 ? 4 : a->group_size == 64 ? 2 : 1;
  // Precedence, first taker wins:
  //   stream-K 256 x 256 > GEMV > K-sliced > lean small-M > M128 > 256 x 256 > 256 x 128 > general
  // (the last three are plan_tiled's row tiles 16 / 8 / <= 4).  The row ranges of the first five overlap only
  // at M <= 4 (GEMV before the K-sliced stream, which never took a call the GEMV could) and at M <= 32 (the
  // K-sliced stream before the lean one).
  const bool taken = plan_xl_sk(a, s, pl) || plan_gemv(a, s, pl) || plan_ks_one_tile(a, s, pl) ||
                     plan_ks_two_tiles(a, s, pl) || plan_small(a, s, pl) || plan_m128(a, s, pl) || plan_tiled(a, s, pl);
  (void)taken;  // (plan_tiled never steps aside)
  pl->part_bytes = pl->split_k > 1 ? (size_t)pl->split_k * a->M * a->N * sizeof(float) : 0;
  if (pl->kernel == W4Kernel::XL_SK) pl->part_bytes = W4_XL_SK_WGS * W4_XL_SK_SLOT_BYTES + W4_XL_SK_SYNC_BYTES;
  pl->aperm_bytes = a->perm ? (((size_t)a->M * a->K * 2 + 255) & ~(size_t)255) : 0;
  return SLM_OK;
}

}  // namespace slm

using namespace slm;

extern "C" {

SLM_API size_t slm_w4a16_gemm_workspace_bytes(const slm_w4_gemm_args* a) {
  GemmPlan pl;
  return plan_gemm(a, &pl) == SLM_OK ? pl.part_bytes + pl.aperm_bytes : 0;
}

SLM_API int32_t slm_w4a16_gemm_deferred_splits(const slm_w4_gemm_args* a) {
  GemmPlan pl;
  return plan_gemm(a, &pl) == SLM_OK && (a->flags & SLM_W4_DEFER_REDUCE) && !a->bias && pl.split_k > 1 ? pl.split_k : 0;
}

SLM_API int32_t slm_w4a16_gemv_norm_supported(const slm_w4_gemm_args* a) {
  GemmPlan pl;
  return plan_gemm(a, &pl) == SLM_OK && pl.kernel == W4Kernel::GEMV && !a->perm &&
         gemv_supported(a->M, a->K, a->group_size, true);
}

SLM_API int slm_w4a16_gemm_plan(const slm_w4_gemm_args* a, slm_w4_plan_info* out) {
  GemmPlan pl;
  if (!out) return SLM_ERR_INVALID_ARG;
  const int rc = plan_gemm(a, &pl);
  if (rc != SLM_OK) return rc;
  *out = slm_w4_plan_info{};
  out->kernel = (int32_t)pl.kernel;
  out->n_mblocks = pl.n_mblocks; out->n_nblocks = pl.n_nblocks;
  out->split_k = pl.split_k; out->chunks_per_split = pl.chunks_per_split;
  out->lds_bytes = pl.lds_bytes; out->part_bytes = pl.part_bytes; out->aperm_bytes = pl.aperm_bytes;
  auto variant = [&](int v0, int v1, int v2, int v3) {
    out->variant[0] = v0; out->variant[1] = v1; out->variant[2] = v2; out->variant[3] = v3;
  };
  switch (pl.kernel) {
    case W4Kernel::GEMV: out->row_tiles = 0; break;
    case W4Kernel::SMALL: out->row_tiles = 1; break;
    case W4Kernel::KS: out->row_tiles = pl.ks.mt; variant(pl.ks.mt, pl.ks.cw, pl.ks.nw, pl.ks.tpw); break;
    case W4Kernel::GENERAL:
      out->row_tiles = pl.general.mt;
      variant(pl.general.mt, pl.general.ntw, pl.general.pc, pl.general.post);
      break;
    case W4Kernel::M128: out->row_tiles = 4; variant(pl.m128.wd, pl.m128.kw, pl.m128.ct, pl.m128.adma); break;
    case W4Kernel::WS: case W4Kernel::XL: out->row_tiles = 8; break;
    case W4Kernel::XL_SK: out->row_tiles = 8; variant(pl.xl_sk.sk_per, 0, 0, 0); break;
  }
  return SLM_OK;
}

}  // extern "C"
