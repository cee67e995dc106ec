// rejection.hip -- validation of speculative drafts in two launches (include/slm_hip.h section 9).
//
//  slm_rejection_sample  <- RejectionSampler::forward / random_sample / greedy_sample
//                           (reference src/speculative/rejection_sampler.cpp:22-226), which build it from
//                           about ten fp32 [bs, k(+1), vocab] torch tensors and two host syncs.
//
// Plan (the call is HBM-bound: it is built from the bytes it must move):
//   launch 1  one 1024-thread workgroup per (sequence, row): rows 0..k-1, plus row k when logprobs are
//             wanted.  The target row streams ONCE with 16-byte loads: online max + rescaled sum, the
//             greedy argmax, then p_d / q_d and the acceptance decision (thread 0).  A 16-byte record
//             (m, S, argmax, accepted) goes to the workspace; top-n (radix select) only with logprobs.
//             Rows of sampled sequences in probability form need no pass at all: p_d is one load.
//   launch 2  the race argmax_i max(p_i - q_i, 0) / E_i.  Masked without logprobs only the first
//             rejected row of a sequence needs it: one workgroup per sequence reads one target and one
//             draft row.  Otherwise (every rejected row's token is an output) one workgroup per (s, j).
//             E_i: one Philox block per 4 consecutive ids (philox.h).  Launch 2 writes every output
//             but the top-n.
// Arithmetic is IEEE fp32 without contraction, division correctly rounded; every argmax is a max over
// the 64-bit composite (order-preserving key << 32 | ~index), so ties go to the lower index and the
// result does not depend on the reduction order.  No float atomics: bit-identical across repeats.
#include <type_traits>

#include "common.h"

#pragma clang fp contract(off)

#include "philox.h"
#include "vocab_row.h"  // keys, loads, reductions, radix_select, gather_sort_top (shared with sampling.hip)

namespace slm {
namespace {

using namespace vocab_row;

// G consecutive values from id i0 (ids >= V read nothing and give -inf); one 8- or 16-byte load when
// the row is aligned and the group is whole
template <int DT, int G>
__device__ __forceinline__ void load_group(const void* row, int i0, int V, bool vec, float (&v)[G]) {
  static_assert(G * elem_bytes<DT>() == 16 || G * elem_bytes<DT>() == 8, "8- or 16-byte groups");
  if (vec && i0 + G <= V) {
    if constexpr (DT == SLM_F32) {
      if constexpr (G == 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(row) + i0);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = x[e];
      } else {
        const f32x2 x = *reinterpret_cast<const f32x2*>(reinterpret_cast<const float*>(row) + i0);
        v[0] = x[0];
        v[1] = x[1];
      }
    } else {
      using T = typename std::conditional<DT == SLM_BF16, bf16_tag, f16_tag>::type;
      const uint16_t* p = reinterpret_cast<const uint16_t*>(row) + i0;
      if constexpr (G == 8) {
        const u32x4 x = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
        for (int c = 0; c < 4; ++c) { v[2 * c] = lo_f32<T>(x[c]); v[2 * c + 1] = hi_f32<T>(x[c]); }
      } else {
        const u32x2 x = *reinterpret_cast<const u32x2*>(p);
#pragma unroll
        for (int c = 0; c < 2; ++c) { v[2 * c] = lo_f32<T>(x[c]); v[2 * c + 1] = hi_f32<T>(x[c]); }
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < G; ++e) v[e] = i0 + e < V ? ld<DT>(row, i0 + e) : -INFINITY;
  }
}

struct Rec {  // one row of one sequence, written by launch 1
  float m, s;   // max and sum of expf(l - m) (logits form)
  int32_t t;    // argmax (lowest index on ties)
  int32_t acc;  // accepted (rows < k)
};

typedef RowSmem<uint32_t> Smem;  // 32-bit bins: the only select here counts

// top-n of a row (n <= 20) in the order (value desc, index asc), into sm.top_key / top_idx (sorted).
// Each pass of the select re-reads the row (L2 / MALL).
template <int DT>
__device__ void top_n(const void* row, int V, int n, Smem& sm) {
  auto e = [&](int i, uint32_t& k, uint32_t& w) { k = f2key(ld<DT>(row, i)); w = 1; return true; };
  const Filter fn = radix_select<false>(e, V, (uint32_t)(n - 1), -1.f, 0.f, sm);
  gather_sort_top(e, V, n, fn, sm);
  __syncthreads();
}

struct Params {
  const void* target;
  int64_t t_ld_s, t_ld_r;
  const float* draft;
  int64_t d_ld_s, d_ld_r;
  const int32_t* draft_ids;
  const int32_t* bonus;
  const uint8_t* do_sample;
  const uint64_t* seeds;
  const int32_t* positions;
  const float* uniform;
  int32_t* next_tokens;
  int32_t* acc_lens;
  float *logprobs, *top_lp;
  int32_t* top_tok;
  int32_t k, V, n_top, probs_form;
  int32_t mask;
  int32_t rows1;     // rows per sequence in launch 1: k, or k + 1 with logprobs
  int32_t race_all;  // launch 2: one workgroup per (s, j) rather than per s
  Rec* rec;          // [n_seqs, k + 1]
};

__device__ __forceinline__ bool sampled(const Params& p, int s) {
  return p.draft && p.do_sample && p.do_sample[s] != 0;
}
template <int DT>
__device__ __forceinline__ const void* target_row(const Params& p, int s, int j) {
  return reinterpret_cast<const char*>(p.target) + ((int64_t)s * p.t_ld_s + (int64_t)j * p.t_ld_r) * elem_bytes<DT>();
}

// ---- launch 1: one workgroup per (s, row) ------------------------------------------------------
template <int DT, bool LP>
__global__ void __launch_bounds__(kThreads) accept_kernel(const Params p) {
  __shared__ Smem sm;
  constexpr int G = 16 / elem_bytes<DT>();
  const int tid = threadIdx.x;
  const int s = blockIdx.x / p.rows1, j = blockIdx.x % p.rows1;
  const int V = p.V;
  const void* row = target_row<DT>(p, s, j);
  const bool samp = sampled(p, s);
  const bool need_sum = !p.probs_form && (samp || LP);
  const bool need_max = !p.probs_form || !samp;  // probability form, sampled: p_d is one load

  float m = -INFINITY, sum = 0.f;
  u64 best = 0;
  if (need_max) {
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    int bi = -1;
    for (int i0 = tid * G; i0 < V; i0 += kThreads * G) {
      float v[G];
      load_group<DT, G>(row, i0, V, vec, v);
      if (bi < 0) bi = i0;  // the thread's lowest id: the argmax of an all -inf run
#pragma unroll
      for (int e = 0; e < G; ++e) {
        const float x = v[e];  // ids >= V are -inf: they never exceed m nor add to the sum
        if (x > m) {
          if (need_sum) sum = sum * expf(m - x);
          m = x;
          bi = i0 + e;
        }
        if (need_sum && x != -INFINITY) sum += expf(x - m);
      }
    }
    best = bi >= 0 ? composite(m, bi) : 0ull;
    best = block_max_u64(best, sm);
    const float mb = key2f((uint32_t)(best >> 32));
    if (need_sum) sum = block_sum_f(sum == 0.f ? 0.f : sum * expf(m - mb), sm);
    m = mb;
  }
  if (tid == 0) {
    Rec r{m, sum, composite_index(best), 0};
    if (j < p.k) {
      const int d = p.draft_ids[(int64_t)s * p.k + j];
      if (samp) {
        if (d >= 0 && d < V) {
          const float pd = p.probs_form ? reinterpret_cast<const float*>(row)[d] : expf(ld<DT>(row, d) - m) / sum;
          const float qd = p.draft[(int64_t)s * p.d_ld_s + (int64_t)j * p.d_ld_r + d];
          const float ratio = pd / qd;
          float u;
          if (p.uniform) {
            u = p.uniform[(int64_t)s * p.k + j];
          } else {
            const uint64_t seed = p.seeds ? p.seeds[s] : 0ull;
            const uint32_t pos = (p.positions ? (uint32_t)p.positions[s] : 0u) + (uint32_t)j;
            u = uniform24(philox_block(seed, pos, 1u, 0u).w[0]);
          }
          r.acc = u < ratio ? 1 : 0;  // NaN rejects
        }
      } else {
        r.acc = r.t == d ? 1 : 0;
      }
    }
    p.rec[(int64_t)s * (p.k + 1) + j] = r;
  }
  if constexpr (LP) {
    if (p.n_top > 0) {
      top_n<DT>(row, V, p.n_top, sm);
      if (tid < p.n_top) {
        const float lse = logf(sum);
        const float x = key2f(sm.top_key[tid]);
        const int64_t o = ((int64_t)s * (p.k + 1) + j) * p.n_top + tid;
        p.top_lp[o] = x == -INFINITY ? -INFINITY : (x - m) - lse;
        p.top_tok[o] = sm.top_idx[tid];
      }
    }
  }
}

// ---- launch 2: the race and the outputs ---------------------------------------------------------
// the recovered token of row j of sequence s: argmax_i max(p_i - q_i, 0) / E_i
template <int DT>
__device__ int race(const Params& p, int s, int j, const Rec& R, Smem& sm) {
  const int tid = threadIdx.x, V = p.V;
  const void* trow = target_row<DT>(p, s, j);
  const float* drow = p.draft + (int64_t)s * p.d_ld_s + (int64_t)j * p.d_ld_r;
  const bool vec = (reinterpret_cast<uintptr_t>(trow) & (4 * elem_bytes<DT>() - 1)) == 0 &&
                   (reinterpret_cast<uintptr_t>(drow) & 15) == 0;
  const uint64_t seed = p.seeds ? p.seeds[s] : 0ull;
  const uint32_t pos = (p.positions ? (uint32_t)p.positions[s] : 0u) + (uint32_t)j;
  u64 best = 0;
  for (int q = tid; q * 4 < V; q += kThreads) {
    const int i0 = 4 * q;
    float tv[4], dv[4];
    load_group<DT, 4>(trow, i0, V, vec, tv);
    load_group<SLM_F32, 4>(drow, i0, V, vec, dv);
    const PhiloxBlock b = philox_block(seed, pos, 2u, (uint32_t)q);  // E of ids i0 .. i0 + 3
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (i0 + e < V) {
        const float pi = p.probs_form ? tv[e] : expf(tv[e] - R.m) / R.s;
        float dd = pi - dv[e];
        dd = dd > 0.f ? dd : 0.f;
        const u64 c = composite(dd / exp_draw(b.w[e]), i0 + e);
        best = c > best ? c : best;
      }
    }
  }
  return composite_index(block_max_u64(best, sm));  // a zero row: id 0
}

template <int DT>
__device__ __forceinline__ float logprob_at(const Params& p, int s, int j, const Rec& R, int tok) {
  if (tok < 0 || tok >= p.V) return NAN;
  return (ld<DT>(target_row<DT>(p, s, j), tok) - R.m) - logf(R.s);
}

template <int DT>
__global__ void __launch_bounds__(kThreads) race_kernel(const Params p) {
  __shared__ Smem sm;
  const int tid = threadIdx.x, k = p.k;
  const int per = p.race_all ? k : 1;
  const int s = blockIdx.x / per, g = blockIdx.x % per;
  const Rec* rec = p.rec + (int64_t)s * (k + 1);
  int f = k;  // the first rejected row
  for (int j = 0; j < k; ++j)
    if (!rec[j].acc) { f = j; break; }
  const int r = p.race_all ? g : f;
  int tok = -1;
  if (r < k) {
    const Rec R = rec[r];
    if (R.acc) tok = p.draft_ids[(int64_t)s * k + r];
    else if (sampled(p, s)) tok = race<DT>(p, s, r, R, sm);
    else tok = R.t;
  }
  int32_t* out = p.next_tokens + (int64_t)s * (k + 1);
  const int bonus = p.bonus[s];
  if (!p.race_all) {  // masked: this workgroup writes the whole sequence
    if (tid <= k) {
      const int jj = tid;
      out[jj] = jj < f ? p.draft_ids[(int64_t)s * k + jj] : jj > f ? -1 : (f < k ? tok : bonus);
    }
    if (tid == 0 && p.acc_lens) p.acc_lens[s] = f + 1;
    return;
  }
  if (tid == 0) {
    out[r] = (p.mask && r > f) ? -1 : tok;
    if (p.logprobs) p.logprobs[(int64_t)s * (k + 1) + r] = logprob_at<DT>(p, s, r, rec[r], tok);
    if (g == 0) {
      out[k] = (p.mask && f < k) ? -1 : bonus;
      if (p.acc_lens) p.acc_lens[s] = f + 1;
      if (p.logprobs) p.logprobs[(int64_t)s * (k + 1) + k] = logprob_at<DT>(p, s, k, rec[k], bonus);
    }
  }
}

int validate(const slm_rejection_args* a) {
  if (!a || a->n_seqs < 0) return SLM_ERR_INVALID_ARG;
  if (a->n_seqs == 0) return SLM_OK;
  if (!a->draft_token_ids || !a->target || !a->bonus_token_ids || !a->next_tokens) return SLM_ERR_INVALID_ARG;
  if (a->k < 1 || a->k > SLM_REJECTION_MAX_K) return SLM_ERR_INVALID_ARG;
  if (a->dtype != SLM_F16 && a->dtype != SLM_BF16 && a->dtype != SLM_F32) return SLM_ERR_UNSUPPORTED;
  if (a->target_is_probs && a->dtype != SLM_F32) return SLM_ERR_UNSUPPORTED;
  if (a->vocab < 1) return SLM_ERR_INVALID_ARG;
  if (a->vocab > kMaxVocab) return SLM_ERR_UNSUPPORTED;
  if (a->n_top < 0 || a->n_top > SLM_SAMPLE_MAX_TOP || a->n_top > a->vocab) return SLM_ERR_INVALID_ARG;
  if (a->n_top > 0 && (!a->top_logprobs || !a->top_tokens)) return SLM_ERR_INVALID_ARG;
  if (a->target_is_probs && (a->logprobs || a->n_top > 0)) return SLM_ERR_INVALID_ARG;
  // the inputs are only read: rows of different sequences may interleave or coincide
  if (a->target_row_stride < a->vocab || a->target_seq_stride < 0) return SLM_ERR_INVALID_ARG;
  if (a->draft_probs && (a->draft_row_stride < a->vocab || a->draft_seq_stride < 0)) return SLM_ERR_INVALID_ARG;
  return SLM_OK;
}

size_t workspace_bytes(const slm_rejection_args* a) {
  if (!a || a->n_seqs <= 0 || a->k < 1 || a->k > SLM_REJECTION_MAX_K) return 0;
  return ((size_t)a->n_seqs * (size_t)(a->k + 1) * sizeof(Rec) + 255) & ~(size_t)255;
}

int launch(const slm_rejection_args* a, void* stream) {
  const int rc = validate(a);
  if (rc != SLM_OK || a->n_seqs == 0) return rc;
  const size_t need = workspace_bytes(a);
  if (!a->workspace || a->workspace_bytes < need) return SLM_ERR_WORKSPACE;
  Params p{};
  p.target = a->target; p.t_ld_s = a->target_seq_stride; p.t_ld_r = a->target_row_stride;
  p.draft = a->draft_probs; p.d_ld_s = a->draft_seq_stride; p.d_ld_r = a->draft_row_stride;
  p.draft_ids = a->draft_token_ids; p.bonus = a->bonus_token_ids;
  p.do_sample = a->do_sample; p.seeds = a->seeds; p.positions = a->positions; p.uniform = a->uniform;
  p.next_tokens = a->next_tokens; p.acc_lens = a->accepted_lens;
  p.logprobs = a->logprobs; p.top_lp = a->top_logprobs; p.top_tok = a->top_tokens; p.n_top = a->n_top;
  p.k = a->k; p.V = a->vocab; p.probs_form = a->target_is_probs ? 1 : 0; p.mask = a->mask_out_rejected ? 1 : 0;
  const bool lp = a->logprobs || a->n_top > 0;
  p.rows1 = a->k + (lp ? 1 : 0);
  p.race_all = (!p.mask || lp) ? 1 : 0;
  p.rec = reinterpret_cast<Rec*>(a->workspace);
  const dim3 g1((unsigned)((int64_t)a->n_seqs * p.rows1)), g2((unsigned)((int64_t)a->n_seqs * (p.race_all ? a->k : 1)));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hip_clear_error();
  auto go = [&](auto k1, auto k2) {
    hipLaunchKernelGGL(k1, g1, dim3(kThreads), 0, s, p);
    hipLaunchKernelGGL(k2, g2, dim3(kThreads), 0, s, p);
  };
  switch (a->dtype) {
    case SLM_F16:
      lp ? go(accept_kernel<SLM_F16, true>, race_kernel<SLM_F16>) : go(accept_kernel<SLM_F16, false>, race_kernel<SLM_F16>);
      break;
    case SLM_BF16:
      lp ? go(accept_kernel<SLM_BF16, true>, race_kernel<SLM_BF16>)
         : go(accept_kernel<SLM_BF16, false>, race_kernel<SLM_BF16>);
      break;
    default:
      lp ? go(accept_kernel<SLM_F32, true>, race_kernel<SLM_F32>) : go(accept_kernel<SLM_F32, false>, race_kernel<SLM_F32>);
      break;
  }
  return hip_check_launch();
}

}  // namespace
}  // namespace slm

extern "C" {

SLM_API size_t slm_rejection_sample_workspace_bytes(const slm_rejection_args* a) { return slm::workspace_bytes(a); }

SLM_API int slm_rejection_sample(const slm_rejection_args* a, void* stream) { return slm::launch(a, stream); }

}  // extern "C"
