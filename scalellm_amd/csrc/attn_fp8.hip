// attn_fp8.hip -- fp8 (e4m3fn) paged KV cache for gfx950: quantising append and token-major stream attention
// (include/slm_hip.h section 27).
//
// The decode step at long context is bound by the KV stream (attn.hip runs at the HBM rate with HBM traffic equal to
// the algorithmic bytes), so the only thing left to take out of it is the bytes: one e4m3 code per element, one static
// fp32 scale per KV head.  Designed for 1-byte rows, not as a parameter of attn_token_kernel:
//
//  * work items as in attn.hip: one workgroup = (query token, group of KV heads, q-head chunk, KV split) with the
//    per-token visible range [lo, hi), so decode, verify and prefill chunks are one kernel (only q_len = 1 is fast);
//  * a lane's 16-byte load holds 16 dims, so LPR = head_dim / 16 lanes share a row (8 at D = 128) and a wave load covers
//    64 / LPR (slot, KV head) units -- with 8 KV heads of 128 one wave load is one slot's whole 1 KiB row.  Every
//    wave of the workgroup works on the same KV heads at its own row phase (up to 8 waves: a byte row is half as
//    long, so twice the rows must be in flight for the same bytes);
//  * U-deep register ring of K and V loads, no LDS on the data path; the block-table slice is staged in LDS;
//  * codes -> T exactly, two per v_cvt_scalef32_pk_{bf16,f16}_fp8 at scale 1.0 (fp8_cvt.h); scores and P.V on dot2
//    with fp32 accumulation.  For P.V the bytes of two rows are interleaved (v_perm) BEFORE the convert, so one
//    convert yields the (row a, row b) pair of a dim that dot2 multiplies with the (p_a, p_b) pair;
//  * no element is ever multiplied by a scale: k_scale[h] is folded into the score scale (soft cap: into the
//    pre-scale), v_scale[h] into the final 1 / l (split: into what the combine kernel writes);
//  * online softmax in base 2, running max in log2 units, rescale of O only when a max moved in the wave (alpha = 1
//    otherwise: the skip changes no bit), past-the-end rows re-read the last valid row and are masked to -inf -- no
//    byte of a slot the sequence does not own is ever loaded, so NaN codes there cannot reach an output;
//  * split-KV: the classic partition (every sequence cut into n_splits ranges), partials in attn.hip's layout, and a
//    small combine kernel of its own that applies v_scale.
#include "attn_common.h"
#include "fp8_cvt.h"
#include "tuning.h"

namespace slm {

struct Attn8Params {
  void* out;
  const void* q;
  const char* kc;
  const char* vc;
  int64_t o_ts, o_hs, q_ts, q_hs, k_hs, v_hs;  // strides in elements (caches: bytes)
  uint32_t k_sb, v_sb;                         // slot strides in bytes (< 2^32: plan_attn8 checks)
  const int* q_cu;
  const int* kv_cu;
  const int* bt;
  const int* bcu;
  const float* k_scale;
  const float* v_scale;
  float* o_part;   // [n_tokens, n_heads, n_splits, head_dim]
  float* ml_part;  // [n_tokens, n_heads, n_splits, 2]
  int batch, n_tokens, n_heads, head_dim;
  int block_shift, block_mask;
  int group, n_chunks, hpw_shift, nhgb, n_splits, window;
  float scale_log2;  // (softcap > 0 ? softcap : sm_scale) * log2(e)
  float pre_scale;   // sm_scale / softcap (softcap > 0 only)
};

constexpr int ATTN8_OD = 16;  // dims per lane
constexpr int ATTN8_MAX_SPLITS = 256;

__device__ __forceinline__ u32x4 ld16nt(const char* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}

// FX: the logits soft cap is compiled in
template <typename T, int LPR, int GC, int U, bool FX>
__global__ void __launch_bounds__(512) attn8_token_kernel(const Attn8Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* tbl = reinterpret_cast<int*>(smem);
  float* xch = reinterpret_cast<float*>(smem + ATTN_TBL_ENT * sizeof(int));

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;

  int bid = blockIdx.x;
  const int split = bid % p.n_splits;
  bid /= p.n_splits;
  const int chunk = bid % p.n_chunks;
  bid /= p.n_chunks;
  const int hgb = bid % p.nhgb;
  const int tok = bid / p.nhgb;

  // token -> sequence: q_cu[b] <= tok < q_cu[b + 1]; a pure-decode batch (q_cu[i] == i) with two independent loads
  int b;
  const int tq0 = p.q_cu[min(tok, p.batch)], tq1 = p.q_cu[min(tok + 1, p.batch)];
  if (tok < p.batch && tq0 == tok && tq1 == tok + 1) {
    b = tok;
  } else {
    int lo_b = 0, hi_b = p.batch;
    while (lo_b < hi_b) {
      const int mid = (lo_b + hi_b) >> 1;
      if (p.q_cu[mid + 1] <= tok)
        lo_b = mid + 1;
      else
        hi_b = mid;
    }
    b = lo_b;
  }
  if (b >= p.batch) return;  // graph-padding row behind q_cu[batch]: untouched

  // lane / wave decomposition: a wave load is HPW KV heads x RPW consecutive rows, the waves are row phases
  constexpr int UPW = 64 / LPR;
  const int g = lane / LPR;
  const int sub = lane % LPR;
  const int hsub = g & ((1 << p.hpw_shift) - 1);
  const int rsub = g >> p.hpw_shift;
  const int RPW = UPW >> p.hpw_shift;
  const int RPI = nw * RPW;  // rows per workgroup iteration

  const int kvh = (hgb << p.hpw_shift) + hsub;
  const int qh0 = kvh * p.group + chunk * GC;
  const char* kbase = p.kc + (int64_t)kvh * p.k_hs + sub * 16;
  const char* vbase = p.vc + (int64_t)kvh * p.v_hs + sub * 16;
  const uint32_t k_sb = p.k_sb, v_sb = p.v_sb;
  // the scales of this lane's KV head, folded into the score transform and the normalisation
  const float ks = p.k_scale[kvh], vs = p.v_scale[kvh];
  const float sl2 = FX ? p.scale_log2 : p.scale_log2 * ks;
  const float pre = p.pre_scale * ks;

  const int q_start = p.q_cu[b];
  const int q_len = p.q_cu[b + 1] - q_start;
  const int kv_len = p.kv_cu[b + 1] - p.kv_cu[b];
  const int diag = kv_len - q_len + (tok - q_start);  // last visible kv index (causal)
  const int hi = min(diag + 1, kv_len);
  const int lo = (p.window >= 0) ? max(0, diag - p.window) : 0;
  const int len = max(hi - lo, 0);
  int per = (len + p.n_splits - 1) / p.n_splits;
  per = ((per + RPI - 1) / RPI) * RPI;  // split ranges are whole workgroup iterations
  const int s_lo = lo + split * per;
  const int s_hi = min(hi, s_lo + per);

  // q fragment: GC heads x 16 dims (packed pairs)
  uint32_t qv[GC][8];
#pragma unroll
  for (int h = 0; h < GC; ++h) {
    const char* ptr = reinterpret_cast<const char*>(p.q) +
                      2 * ((int64_t)tok * p.q_ts + (int64_t)(qh0 + h) * p.q_hs + sub * 16);
    const u32x4 t0 = *reinterpret_cast<const u32x4*>(ptr), t1 = *reinterpret_cast<const u32x4*>(ptr + 16);
    qv[h][0] = t0.x; qv[h][1] = t0.y; qv[h][2] = t0.z; qv[h][3] = t0.w;
    qv[h][4] = t1.x; qv[h][5] = t1.y; qv[h][6] = t1.z; qv[h][7] = t1.w;
  }

  constexpr int OD = ATTN8_OD;
  float m[GC], l[GC], o[GC][OD];
#pragma unroll
  for (int h = 0; h < GC; ++h) {
    m[h] = ATTN_M_INIT;
    l[h] = 0.f;
#pragma unroll
    for (int j = 0; j < OD; ++j) o[h][j] = 0.f;
  }

  const int bcu0 = p.bcu[b];
  u32x4 kr[U], vr[U];

  for (int c_lo = s_lo; c_lo < s_hi;) {
    const int blk0 = c_lo >> p.block_shift;
    const int blk_end = min(((s_hi - 1) >> p.block_shift) + 1, blk0 + ATTN_TBL_ENT);
    const int c_hi = min(s_hi, blk_end << p.block_shift);
    __syncthreads();
    for (int e = tid; e < blk_end - blk0; e += blockDim.x) tbl[e] = p.bt[bcu0 + blk0 + e];
    __syncthreads();

    const int wrow0 = c_lo + wave * RPW;  // wave-uniform first row of this wave in iteration 0
    const int n_it = (c_hi - c_lo + RPI - 1) / RPI;

    // U rows per lane group per trip, branch-free on the data path: loads are unconditional with clamped rows (a
    // past-the-end row re-reads the last valid row of the range and is masked), the next batch's K load is issued as
    // each K register is consumed, the V loads as each V pair is consumed
    int slot_n[U];
    auto slots_for = [&](int it0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = min(wrow0 + (it0 + u) * RPI + rsub, c_hi - 1);
        slot_n[u] = tbl[(row >> p.block_shift) - blk0] + (row & p.block_mask);
      }
    };
    slots_for(0);
#pragma unroll
    for (int u = 0; u < U; ++u) kr[u] = ld16nt(kbase + (uint64_t)(uint32_t)slot_n[u] * k_sb);
#pragma unroll
    for (int u = 0; u < U; ++u) vr[u] = ld16nt(vbase + (uint64_t)(uint32_t)slot_n[u] * v_sb);
    asm volatile("" ::: "memory");  // the prologue loads stay in front of the loop

    for (int it0 = 0; it0 < n_it; it0 += U) {
      slots_for(it0 + U);  // next batch (clamped past the end)
      float s[U][GC];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const u32x4 kk = kr[u];
        const uint32_t kt[8] = {fp8x2_to_t<T, false>(kk.x), fp8x2_to_t<T, true>(kk.x), fp8x2_to_t<T, false>(kk.y),
                                fp8x2_to_t<T, true>(kk.y),  fp8x2_to_t<T, false>(kk.z), fp8x2_to_t<T, true>(kk.z),
                                fp8x2_to_t<T, false>(kk.w), fp8x2_to_t<T, true>(kk.w)};
#pragma unroll
        for (int h = 0; h < GC; ++h) {
          float a = dot2<T>(kt[0], qv[h][0], 0.f);
#pragma unroll
          for (int j = 1; j < 8; ++j) a = dot2<T>(kt[j], qv[h][j], a);
          s[u][h] = a;
        }
        kr[u] = ld16nt(kbase + (uint64_t)(uint32_t)slot_n[u] * k_sb);
        __builtin_amdgcn_sched_barrier(0);  // pin: the next batch's K load issues right here
      }
      group_sum_many<LPR, U * GC>(&s[0][0]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool valid = wrow0 + (it0 + u) * RPI + rsub < c_hi;
#pragma unroll
        for (int h = 0; h < GC; ++h) {
          float a = s[u][h];
          if constexpr (FX) a = fast_tanh(a * pre);
          s[u][h] = valid ? a * sl2 : -INFINITY;
        }
      }
      // one running-max update per batch of U rows; O is rescaled only when some max of the wave moved
      float mn[GC];
      bool moved = false;
#pragma unroll
      for (int h = 0; h < GC; ++h) {
        mn[h] = m[h];
#pragma unroll
        for (int u = 0; u < U; ++u) mn[h] = fmaxf(mn[h], s[u][h]);
        moved |= mn[h] > m[h];
      }
      if (__builtin_amdgcn_ballot_w64(moved) != 0) {
#pragma unroll
        for (int h = 0; h < GC; ++h) {
          const float alpha = fast_exp2(m[h] - mn[h]);
          m[h] = mn[h];
          l[h] *= alpha;
#pragma unroll
          for (int j = 0; j < OD; ++j) o[h][j] *= alpha;
        }
      }
      float pr[U][GC];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int h = 0; h < GC; ++h) {
          pr[u][h] = fast_exp2(s[u][h] - m[h]);
          l[h] += pr[u][h];
        }
      // P.V over row pairs: the code bytes of rows a and b are interleaved per dim, one convert gives the dim's
      // (a, b) pair in T, P is rounded to T
#pragma unroll
      for (int u = 0; u < U; u += 2) {
        uint32_t pp[GC];
#pragma unroll
        for (int h = 0; h < GC; ++h) pp[h] = pack2<T>(pr[u][h], pr[u + 1][h]);
        const u32x4 va = vr[u], vb = vr[u + 1];
        const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t x0 = __builtin_amdgcn_perm(wb[j], wa[j], 0x05010400u);  // a0 b0 a1 b1
          const uint32_t x1 = __builtin_amdgcn_perm(wb[j], wa[j], 0x07030602u);  // a2 b2 a3 b3
          const uint32_t vt[4] = {fp8x2_to_t<T, false>(x0), fp8x2_to_t<T, true>(x0), fp8x2_to_t<T, false>(x1),
                                  fp8x2_to_t<T, true>(x1)};
#pragma unroll
          for (int h = 0; h < GC; ++h) {
#pragma unroll
            for (int d = 0; d < 4; ++d) o[h][4 * j + d] = dot2<T>(vt[d], pp[h], o[h][4 * j + d]);
          }
        }
        vr[u] = ld16nt(vbase + (uint64_t)(uint32_t)slot_n[u] * v_sb);
        vr[u + 1] = ld16nt(vbase + (uint64_t)(uint32_t)slot_n[u + 1] * v_sb);
        __builtin_amdgcn_sched_barrier(0);  // pin: the next batch's V loads issue right here
      }
      asm volatile("" ::: "memory");
    }
    c_lo = c_hi;
  }

  // ---- merge the row-phase lane groups of this wave (same KV head, different rows) ----
  auto merge = [&](const float (&om)[GC], const float (&ol)[GC], const float (&oo)[GC][OD]) {
#pragma unroll
    for (int h = 0; h < GC; ++h) {
      const float mx = fmaxf(m[h], om[h]);
      const float fa = fast_exp2(m[h] - mx);
      const float fb = fast_exp2(om[h] - mx);
      m[h] = mx;
      l[h] = l[h] * fa + ol[h] * fb;
#pragma unroll
      for (int j = 0; j < OD; ++j) o[h][j] = o[h][j] * fa + oo[h][j] * fb;
    }
  };
  for (int d = LPR << p.hpw_shift; d < 64; d <<= 1) {
    float om[GC], ol[GC], oo[GC][OD];
#pragma unroll
    for (int h = 0; h < GC; ++h) {
      om[h] = __shfl_xor(m[h], d, 64);
      ol[h] = __shfl_xor(l[h], d, 64);
#pragma unroll
      for (int j = 0; j < OD; ++j) oo[h][j] = __shfl_xor(o[h][j], d, 64);
    }
    merge(om, ol, oo);
  }

  // ---- merge the waves through LDS (sequential rounds, fixed order; once per workgroup) ----
  constexpr int SF = 2 + OD;  // floats of state per lane and head
  for (int r = 1; r < nw; ++r) {
    __syncthreads();
    if (wave == r) {
#pragma unroll
      for (int h = 0; h < GC; ++h) {
        xch[(h * SF + 0) * 64 + lane] = m[h];
        xch[(h * SF + 1) * 64 + lane] = l[h];
#pragma unroll
        for (int j = 0; j < OD; ++j) xch[(h * SF + 2 + j) * 64 + lane] = o[h][j];
      }
    }
    __syncthreads();
    if (wave == 0) {
      float om[GC], ol[GC], oo[GC][OD];
#pragma unroll
      for (int h = 0; h < GC; ++h) {
        om[h] = xch[(h * SF + 0) * 64 + lane];
        ol[h] = xch[(h * SF + 1) * 64 + lane];
#pragma unroll
        for (int j = 0; j < OD; ++j) oo[h][j] = xch[(h * SF + 2 + j) * 64 + lane];
      }
      merge(om, ol, oo);
    }
  }

  if (wave == 0 && rsub == 0) {
    if (p.n_splits == 1) {
#pragma unroll
      for (int h = 0; h < GC; ++h) {
        const float inv = l[h] > 0.f ? vs / l[h] : 0.f;  // v_scale: here and nowhere else
        float y[OD];
#pragma unroll
        for (int j = 0; j < OD; ++j) y[j] = scaled(o[h][j], inv);
        char* ptr = reinterpret_cast<char*>(p.out) +
                    2 * ((int64_t)tok * p.o_ts + (int64_t)(qh0 + h) * p.o_hs + sub * 16);
        *reinterpret_cast<u32x4*>(ptr) =
            u32x4{pack2<T>(y[0], y[1]), pack2<T>(y[2], y[3]), pack2<T>(y[4], y[5]), pack2<T>(y[6], y[7])};
        *reinterpret_cast<u32x4*>(ptr + 16) =
            u32x4{pack2<T>(y[8], y[9]), pack2<T>(y[10], y[11]), pack2<T>(y[12], y[13]), pack2<T>(y[14], y[15])};
      }
    } else {
#pragma unroll
      for (int h = 0; h < GC; ++h) {
        const int64_t pi = ((int64_t)tok * p.n_heads + (qh0 + h)) * p.n_splits + split;
        float* op = p.o_part + pi * p.head_dim + sub * 16;
#pragma unroll
        for (int j = 0; j < OD; j += 4)
          *reinterpret_cast<f32x4*>(op + j) = f32x4{o[h][j], o[h][j + 1], o[h][j + 2], o[h][j + 3]};
        if (sub == 0) {
          p.ml_part[pi * 2 + 0] = m[h];
          p.ml_part[pi * 2 + 1] = l[h];
        }
      }
    }
  }
}

// out[tok, head, :] = v_scale * sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s: one wave per (tok, head).  Lanes first
// own splits (weights parked in LDS), then 4 dims each.  A split without rows (l = 0) has weight 0.
template <typename T>
__global__ void __launch_bounds__(256) attn8_combine_kernel(const Attn8Params p) {
  __shared__ float wsm[4][ATTN8_MAX_SPLITS];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t item = (int64_t)blockIdx.x * 4 + wv;
  if (item >= (int64_t)p.n_tokens * p.n_heads) return;  // (whole waves leave; no workgroup barrier below)
  const int tok = (int)(item / p.n_heads), head = (int)(item % p.n_heads);
  if (tok >= p.q_cu[p.batch]) return;  // graph-padding row: nobody wrote its partials
  const float* ml = p.ml_part + item * p.n_splits * 2;
  float mreg[4], lreg[4];
  float M = ATTN_M_INIT;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s = lane + 64 * i;
    mreg[i] = ATTN_M_INIT;
    lreg[i] = 0.f;
    if (s < p.n_splits) {
      const float2 v = *reinterpret_cast<const float2*>(ml + 2 * s);
      mreg[i] = v.x;
      lreg[i] = v.y;
    }
    if (lreg[i] > 0.f) M = fmaxf(M, mreg[i]);
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) M = fmaxf(M, __shfl_xor(M, d, 64));
  float L = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float w = lreg[i] > 0.f ? fast_exp2(mreg[i] - M) : 0.f;
    L += w * lreg[i];
    wsm[wv][lane + 64 * i] = w;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) L += __shfl_xor(L, d, 64);
  __builtin_amdgcn_wave_barrier();  // wsm row is wave-private; LDS ops of one wave are ordered

  const int d0 = lane * 4;
  if (d0 >= p.head_dim) return;
  const float* op = p.o_part + item * p.n_splits * p.head_dim + d0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < p.n_splits; ++s)
    acc += wsm[wv][s] * *reinterpret_cast<const f32x4*>(op + (int64_t)s * p.head_dim);
  const float inv = L > 0.f ? p.v_scale[head / p.group] / L : 0.f;  // v_scale: here and nowhere else
  u32x2 r;
  r.x = pack2<T>(scaled(acc.x, inv), scaled(acc.y, inv));
  r.y = pack2<T>(scaled(acc.z, inv), scaled(acc.w, inv));
  *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(p.out) +
                            2 * ((int64_t)tok * p.o_ts + (int64_t)head * p.o_hs + d0)) = r;
}

// cache[slot, h, 16 c .. 16 c + 16) = e4m3(x / s[h]) for K and V: one lane per 16 elements, 16-byte stores
template <typename T>
__global__ void __launch_bounds__(256) kv_fp8_append_kernel(
    const int* __restrict__ slot_ids, const char* __restrict__ keys, const char* __restrict__ values,
    int64_t k_stride_b, int64_t v_stride_b, const float* __restrict__ k_scale, const float* __restrict__ v_scale,
    char* __restrict__ key_cache, char* __restrict__ value_cache, int64_t n_tokens, int row_elems, int head_dim) {
  const int lanes_per_row = row_elems / 16;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t tok = idx / lanes_per_row;
  const int c = (int)(idx % lanes_per_row);
  if (tok >= n_tokens) return;
  const int64_t slot = slot_ids[tok];
  const int h = c * 16 / head_dim;
  auto quant8 = [](const u32x4 x, const float s) {
    float f[8];
    unpack8<T>(x, f);
    u32x2 q;
    q.x = f32x2_to_e4m3<false>(0u, f[0] / s, f[1] / s);
    q.x = f32x2_to_e4m3<true>(q.x, f[2] / s, f[3] / s);
    q.y = f32x2_to_e4m3<false>(0u, f[4] / s, f[5] / s);
    q.y = f32x2_to_e4m3<true>(q.y, f[6] / s, f[7] / s);
    return q;
  };
  auto quant16 = [&](const char* src, const float s, char* dst) {
    const u32x2 q0 = quant8(*reinterpret_cast<const u32x4*>(src), s);
    const u32x2 q1 = quant8(*reinterpret_cast<const u32x4*>(src + 16), s);
    *reinterpret_cast<u32x4*>(dst) = u32x4{q0.x, q0.y, q1.x, q1.y};
  };
  quant16(keys + tok * k_stride_b + c * 32, k_scale[h], key_cache + slot * (int64_t)row_elems + c * 16);
  quant16(values + tok * v_stride_b + c * 32, v_scale[h], value_cache + slot * (int64_t)row_elems + c * 16);
}

// ------------------------------- host side ------------------------------------------
struct Attn8Plan {
  int lpr, gc, n_chunks, hpw, nhgb, nw, n_splits, u;
  int64_t grid;
  size_t lds_bytes, ws_bytes;
};

static int plan_attn8(const slm_attn_fp8_args* a, Attn8Plan* pl) {
  if (!a) return SLM_ERR_INVALID_ARG;
  if (a->n_heads <= 0 || a->n_kv_heads <= 0 || a->n_heads % a->n_kv_heads) return SLM_ERR_INVALID_ARG;
  if (a->n_tokens < 0 || a->batch_size < 0 || a->num_splits < 0) return SLM_ERR_INVALID_ARG;
  if (a->dtype != SLM_F16 && a->dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (a->alibi_slopes != nullptr) return SLM_ERR_UNSUPPORTED;
  if (a->head_dim != 64 && a->head_dim != 128 && a->head_dim != 256) return SLM_ERR_SHAPE;
  if (!is_pow2(a->block_size)) return SLM_ERR_INVALID_ARG;
  // slot stride in bytes below 2^32: one 32 x 32 -> 64-bit multiply per address
  if (a->k_stride[0] <= 0 || a->v_stride[0] <= 0 || a->k_stride[0] >= (1ll << 32) || a->v_stride[0] >= (1ll << 32))
    return SLM_ERR_INVALID_ARG;
  const int D = a->head_dim, G = a->n_heads / a->n_kv_heads;
  pl->lpr = D / 16;
  pl->gc = (G % 4 == 0) ? 4 : (G % 2 == 0) ? 2 : 1;  // 16 output dims per head and lane: 4 heads fill the registers
  pl->n_chunks = G / pl->gc;
  const int upw = 64 / pl->lpr;
  int hpw = 1;
  while (hpw * 2 <= upw && a->n_kv_heads % (hpw * 2) == 0) hpw *= 2;
  // ~256 workgroups per launch, >= 128 KV rows per split; a small batch that cannot fill the chip even with every
  // split takes fewer KV heads per wave load (consecutive rows of them instead): more head groups, more workgroups
  const int64_t target_wgs = 256;
  int64_t max_by_len = (a->max_kv_len > 128 ? a->max_kv_len : 128) / 128;
  if (max_by_len > ATTN8_MAX_SPLITS) max_by_len = ATTN8_MAX_SPLITS;
  auto base_for = [&](int h) { return (int64_t)a->n_tokens * (a->n_kv_heads / h) * pl->n_chunks; };
  while (hpw > 1 && base_for(hpw) * max_by_len < target_wgs) hpw /= 2;
  pl->hpw = hpw;
  pl->nhgb = a->n_kv_heads / hpw;
  const int64_t base = base_for(hpw);
  int64_t want = (target_wgs + base - 1) / (base > 0 ? base : 1);
  if (want > max_by_len) want = max_by_len;
  if (want < 1) want = 1;
  if (a->num_splits > ATTN8_MAX_SPLITS) return SLM_ERR_INVALID_ARG;
  int forced = a->num_splits > 0 ? a->num_splits : tune_get(TUNE_ATTN8_SPLITS, 0);
  if (forced > ATTN8_MAX_SPLITS) forced = ATTN8_MAX_SPLITS;
  pl->n_splits = forced > 0 ? forced : (int)want;
  // a byte row is half as long as a T row: long ranges take 8 waves to keep the bytes in flight (SLM_ATTN8_NW: 4 / 8)
  pl->nw = tune_get(TUNE_ATTN8_NW, (int64_t)a->max_kv_len / pl->n_splits >= 1024 ? 8 : 4);
  if (pl->nw != 4 && pl->nw != 8) pl->nw = 4;
  pl->u = a->logits_soft_cap > 0.f ? 2 : 4;
  pl->lds_bytes = ATTN_TBL_ENT * sizeof(int) + (size_t)(2 + ATTN8_OD) * pl->gc * 64 * sizeof(float);
  pl->grid = base * pl->n_splits;
  if (pl->grid > 0x7fffffffLL) return SLM_ERR_INVALID_ARG;
  pl->ws_bytes = pl->n_splits > 1
                     ? (size_t)a->n_tokens * a->n_heads * pl->n_splits * (a->head_dim + 2) * sizeof(float)
                     : 0;
  return SLM_OK;
}

template <typename T, int LPR, int GC>
static void launch_attn8(const Attn8Params& kp, const Attn8Plan& pl, bool fx, hipStream_t st) {
  const dim3 g((unsigned)pl.grid), blk(pl.nw * 64);
  if (fx)
    hipLaunchKernelGGL((attn8_token_kernel<T, LPR, GC, 2, true>), g, blk, pl.lds_bytes, st, kp);
  else
    hipLaunchKernelGGL((attn8_token_kernel<T, LPR, GC, 4, false>), g, blk, pl.lds_bytes, st, kp);
}

template <typename T, int LPR>
static void dispatch_attn8_gc(const Attn8Params& kp, const Attn8Plan& pl, bool fx, hipStream_t st) {
  switch (pl.gc) {
    case 4: launch_attn8<T, LPR, 4>(kp, pl, fx, st); break;
    case 2: launch_attn8<T, LPR, 2>(kp, pl, fx, st); break;
    default: launch_attn8<T, LPR, 1>(kp, pl, fx, st); break;
  }
}

template <typename T>
static void dispatch_attn8(const Attn8Params& kp, const Attn8Plan& pl, bool fx, hipStream_t st) {
  switch (pl.lpr) {
    case 4: dispatch_attn8_gc<T, 4>(kp, pl, fx, st); break;
    case 8: dispatch_attn8_gc<T, 8>(kp, pl, fx, st); break;
    default: dispatch_attn8_gc<T, 16>(kp, pl, fx, st); break;
  }
}

}  // namespace slm

using namespace slm;

extern "C" {

SLM_API int slm_paged_kv_fp8_attention_plan(const slm_attn_fp8_args* a, slm_attn_fp8_plan_info* out) {
  Attn8Plan pl;
  if (!out) return SLM_ERR_INVALID_ARG;
  const int rc = plan_attn8(a, &pl);
  if (rc != SLM_OK) return rc;
  *out = slm_attn_fp8_plan_info{};
  out->n_splits = pl.n_splits; out->waves = pl.nw; out->lanes_per_row = pl.lpr; out->heads_per_lane = pl.gc;
  out->n_chunks = pl.n_chunks; out->kv_heads_per_wave = pl.hpw;
  out->rows_per_iter = pl.nw * (64 / pl.lpr / pl.hpw); out->ring_depth = pl.u;
  out->grid = pl.grid; out->lds_bytes = pl.lds_bytes; out->workspace_bytes = pl.ws_bytes;
  return SLM_OK;
}

SLM_API int slm_paged_kv_fp8_attention(const slm_attn_fp8_args* a, void* stream) {
  Attn8Plan pl;
  int rc = plan_attn8(a, &pl);
  if (rc != SLM_OK) return rc;
  if (a->n_tokens == 0 || a->batch_size == 0) return SLM_OK;
  if (!a->out || !a->query || !a->key_cache || !a->value_cache || !a->q_cu_lens || !a->kv_cu_lens ||
      !a->block_table || !a->block_cu_lens || !a->k_scale || !a->v_scale)
    return SLM_ERR_INVALID_ARG;
  // 16-byte vector access on rows: bases and strides keep 16-byte alignment (caches: one byte per element)
  if (!aligned16(a->out) || !aligned16(a->query) || !aligned16(a->key_cache) || !aligned16(a->value_cache) ||
      (reinterpret_cast<uintptr_t>(a->k_scale) & 3u) || (reinterpret_cast<uintptr_t>(a->v_scale) & 3u))
    return SLM_ERR_ALIGNMENT;
  for (int i = 0; i < 2; ++i)
    if (a->o_stride[i] % 8 || a->q_stride[i] % 8 || a->k_stride[i] % 16 || a->v_stride[i] % 16)
      return SLM_ERR_ALIGNMENT;
  if (pl.ws_bytes > 0 && (!a->workspace || a->workspace_bytes < pl.ws_bytes)) return SLM_ERR_WORKSPACE;
  if (pl.ws_bytes > 0 && !aligned16(a->workspace)) return SLM_ERR_ALIGNMENT;

  Attn8Params kp;
  kp.out = a->out; kp.q = a->query;
  kp.kc = reinterpret_cast<const char*>(a->key_cache); kp.vc = reinterpret_cast<const char*>(a->value_cache);
  kp.o_ts = a->o_stride[0]; kp.o_hs = a->o_stride[1];
  kp.q_ts = a->q_stride[0]; kp.q_hs = a->q_stride[1];
  kp.k_hs = a->k_stride[1]; kp.v_hs = a->v_stride[1];
  kp.k_sb = (uint32_t)a->k_stride[0]; kp.v_sb = (uint32_t)a->v_stride[0];
  kp.q_cu = a->q_cu_lens; kp.kv_cu = a->kv_cu_lens;
  kp.bt = a->block_table; kp.bcu = a->block_cu_lens;
  kp.k_scale = a->k_scale; kp.v_scale = a->v_scale;
  kp.batch = a->batch_size; kp.n_tokens = a->n_tokens;
  kp.n_heads = a->n_heads; kp.head_dim = a->head_dim;
  kp.block_shift = ilog2(a->block_size); kp.block_mask = a->block_size - 1;
  kp.group = a->n_heads / a->n_kv_heads;
  kp.n_chunks = pl.n_chunks; kp.hpw_shift = ilog2(pl.hpw); kp.nhgb = pl.nhgb;
  kp.n_splits = pl.n_splits; kp.window = a->sliding_window;
  const bool fx = a->logits_soft_cap > 0.f;
  if (fx) {  // softmax(tanh(x * sm_scale / cap) * cap), as section 1
    kp.pre_scale = a->sm_scale / a->logits_soft_cap;
    kp.scale_log2 = a->logits_soft_cap * LOG2E;
  } else {
    kp.pre_scale = 0.f;
    kp.scale_log2 = a->sm_scale * LOG2E;
  }
  kp.o_part = nullptr; kp.ml_part = nullptr;
  if (pl.n_splits > 1) {
    kp.o_part = reinterpret_cast<float*>(a->workspace);
    kp.ml_part = kp.o_part + (size_t)a->n_tokens * a->n_heads * pl.n_splits * a->head_dim;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hip_clear_error();
  dispatch_dtype(a->dtype, [&](auto t) { dispatch_attn8<decltype(t)>(kp, pl, fx, st); });
  rc = hip_check_launch();
  if (rc != SLM_OK || pl.n_splits == 1) return rc;
  const int64_t items = (int64_t)a->n_tokens * a->n_heads;
  dispatch_dtype(a->dtype, [&](auto t) {
    hipLaunchKernelGGL(attn8_combine_kernel<decltype(t)>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, kp);
  });
  return hip_check_launch();
}

SLM_API int slm_kv_fp8_append(const int32_t* slot_ids, const void* keys, const void* values, int64_t k_token_stride,
                              int64_t v_token_stride, const float* k_scale, const float* v_scale, void* key_cache,
                              void* value_cache, int64_t n_tokens, int32_t n_kv_heads, int32_t head_dim,
                              int32_t dtype, void* stream) {
  if (n_tokens < 0 || n_kv_heads <= 0 || head_dim <= 0) return SLM_ERR_INVALID_ARG;
  if (dtype != SLM_F16 && dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (head_dim % 16) return SLM_ERR_SHAPE;
  const int64_t row_elems = (int64_t)n_kv_heads * head_dim;
  if (row_elems > (1 << 24) || n_tokens >= ((int64_t)1 << 31)) return SLM_ERR_INVALID_ARG;
  if (n_tokens == 0) return SLM_OK;
  if (!slot_ids || !keys || !values || !k_scale || !v_scale || !key_cache || !value_cache) return SLM_ERR_INVALID_ARG;
  if (k_token_stride < row_elems || v_token_stride < row_elems) return SLM_ERR_INVALID_ARG;
  if (!aligned16(keys) || !aligned16(values) || !aligned16(key_cache) || !aligned16(value_cache) ||
      k_token_stride % 8 || v_token_stride % 8 || (reinterpret_cast<uintptr_t>(k_scale) & 3u) ||
      (reinterpret_cast<uintptr_t>(v_scale) & 3u) || (reinterpret_cast<uintptr_t>(slot_ids) & 3u))
    return SLM_ERR_ALIGNMENT;
  const int64_t lanes = n_tokens * (row_elems / 16);
  if ((lanes + 255) / 256 > 0x7fffffffLL) return SLM_ERR_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hip_clear_error();
  const dim3 grid((unsigned)((lanes + 255) / 256)), blk(256);
  dispatch_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(kv_fp8_append_kernel<decltype(t)>, grid, blk, 0, st, slot_ids, (const char*)keys,
                       (const char*)values, 2 * k_token_stride, 2 * v_token_stride, k_scale, v_scale,
                       (char*)key_cache, (char*)value_cache, n_tokens, (int)row_elems, (int)head_dim);
  });
  return hip_check_launch();
}

}  // extern "C"
