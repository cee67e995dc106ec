// sampling.hip -- logits processing and sampling in one launch per call (include/slm_hip.h section 8).
//
//  slm_sample          <- LogitsProcessor::create(params) + Sampler::forward as Worker::execute_model
//                         runs them (reference src/engine/worker.cpp:154-187): penalties
//                         (src/kernels/sampling/penalty_kernels.cu:9-143), temperature, top-k / top-p
//                         (src/sampling/logits_processor.h:224-284), softmax + exponential race +
//                         argmax, logprobs and top logprobs (src/sampling/sampler.cpp:19-70).
//  slm_logits_process  <- the processing half alone; in place with penalties only it is
//                         kernel::apply_frequency_presence_penalty / apply_repetition_penalty.
//
// Plan: one 1024-thread workgroup per row; thread t visits tokens t, t + 1024, ... of the row in
// every pass (coalesced, any alignment, any vocab).  Each pass re-reads the row (L2 / MALL):
//   setup   penalised ids -> an LDS bitmap over the vocab + per-word prefix popcounts; the
//           penalised value of each id (steps 1-2) goes to workspace[row][rank of id], so every
//           later pass learns "is token i penalised, and its value" from one LDS word
//   max     block argmax over (value desc, index asc): the greedy token and the softmax shift
//   top-k   radix select, 8-bit digits of the order-preserving key, count histograms
//   top-p   radix select on the same keys with 64-bit fixed-point mass histograms (integer
//           atomics: exact, so the boundary is deterministic)
//           a boundary inside a run of equal keys is resolved lowest-index-first by a radix
//           select over the index
//   sample  the survivors' exp(x - m), their sum (fixed order) and the exponential race
//   top-n   radix select over (kept ? key : key(-inf)), gather n <= 20 into LDS, sort
//   write   probs, then processed logits (last: `processed` may alias `logits`)
// The processing arithmetic is plain IEEE fp32 without contraction (step 1 is a multiply and two
// subtractions, not an FMA) and with correctly rounded division, so numpy float32 reproduces it.
#include "common.h"

#pragma clang fp contract(off)

#include "philox.h"     // philox_word, exp_draw (shared with rejection.hip)
#include "vocab_row.h"  // keys, loads, reductions, radix_select, gather_sort_top (shared with rejection.hip)

namespace slm {
namespace {

using namespace vocab_row;

constexpr int kMaxPenVocab = 1 << 19;         // bitmap + prefix of 2^14 words each: 128 KiB of LDS

struct Smem : RowSmem<u64> {  // 64-bit bins: top-p sums fixed-point masses
  uint32_t scan32[kWaves];
};

// exclusive prefix sum of one uint32 per thread, in thread order
__device__ uint32_t block_excl_scan(uint32_t v, Smem& sm) {
  const int tid = threadIdx.x, lane = tid & 63;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  if (lane == 63) sm.scan32[tid >> 6] = inc;
  __syncthreads();
  uint32_t base = 0;
  for (int w = 0; w < (tid >> 6); ++w) base += sm.scan32[w];
  __syncthreads();
  return base + inc - v;
}

struct Params {
  const void* logits;
  int64_t ld_in;
  int32_t V, max_unique;
  const float *freq, *pres, *rep, *temp, *top_p;
  const int64_t* top_k;
  const int64_t* ids;
  const int32_t *counts, *lens;
  const uint8_t* do_sample;
  const uint64_t* seeds;
  const int32_t* positions;
  int32_t* next_tokens;
  void* processed;
  int64_t ld_out;
  float *probs, *logprobs, *top_lp;
  int32_t* top_tok;
  int32_t n_top;
  int32_t sample;   // 1: slm_sample, 0: slm_logits_process
  int32_t has_pen;  // penalties given (bitmap in dynamic LDS, values in the workspace)
  int32_t sparse;   // in place, penalties only: write the penalised entries and stop
  float* ws;
};

template <int DT>
__global__ void __launch_bounds__(kThreads) sample_kernel(const Params p) {
  __shared__ Smem sm;
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
  const int tid = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int V = p.V;
  const void* row = reinterpret_cast<const char*>(p.logits) + r * p.ld_in * elem_bytes<DT>();
  float inv_t = 1.0f;
  if (p.temp) {
    const float t = p.temp[r];
    inv_t = t == 0.f ? 1.0f : 1.0f / t;  // penalty_kernels.cu:19-22 (IEEE division)
  }
  const int W = (V + 31) >> 5;
  uint32_t* bits = dyn;
  uint32_t* pre = dyn + W;
  float* pval = p.ws + r * (int64_t)p.max_unique;
  bool pen = false;

  // ---- setup: the penalised ids (steps 1-2) ---------------------------------------------------
  if (p.has_pen) {
    int n = p.lens[r];
    n = n < 0 ? 0 : (n > p.max_unique ? p.max_unique : n);
    pen = n > 0;
    if (!pen && p.sparse) return;
    if (pen) {
      const int64_t* ids = p.ids + r * (int64_t)p.max_unique;
      const int32_t* counts = p.counts ? p.counts + r * (int64_t)p.max_unique : nullptr;
      if (!p.sparse) {
        for (int w = tid; w < W; w += kThreads) bits[w] = 0u;
        __syncthreads();
        for (int j = tid; j < n; j += kThreads) {
          const int64_t id = ids[j];
          if (id >= 0 && id < V) atomicOr(&bits[id >> 5], 1u << (id & 31));
        }
        __syncthreads();
        const int chunk = (W + kThreads - 1) / kThreads;
        const int w0 = min(tid * chunk, W), w1 = min(w0 + chunk, W);
        uint32_t c = 0;
        for (int w = w0; w < w1; ++w) c += __popc(bits[w]);
        uint32_t base = block_excl_scan(c, sm);
        for (int w = w0; w < w1; ++w) { pre[w] = base; base += __popc(bits[w]); }
        __syncthreads();
      }
      const float fq = p.freq ? p.freq[r] : 0.f, pr = p.pres ? p.pres[r] : 0.f;
      const float rp = p.rep ? p.rep[r] : 1.f;
      for (int j = tid; j < n; j += kThreads) {
        const int64_t id = ids[j];
        if (id < 0 || id >= V) continue;
        float x = ld<DT>(row, (int)id);
        if (counts && counts[j] > 0) {  // penalty_kernels.cu:135-140
          if (p.freq) x = x - (float)counts[j] * fq;
          if (p.pres) x = x - pr;
        }
        if (p.rep) x = x < 0.0f ? x * rp : x / rp;  // penalty_kernels.cu:76-78
        if (p.sparse) {
          st<DT>(reinterpret_cast<char*>(p.processed) + r * p.ld_out * elem_bytes<DT>(), (int)id, x);
        } else {
          const int iw = (int)(id >> 5);
          const uint32_t b = 1u << (id & 31);
          pval[pre[iw] + __popc(bits[iw] & (b - 1u))] = x;
        }
      }
      if (p.sparse) return;
      __syncthreads();  // workgroup-scope release / acquire: pval is visible to every thread
    }
  }
  auto proc = [&](int i) -> float {
    if (pen) {
      const uint32_t w = bits[i >> 5], b = 1u << (i & 31);
      if (w & b) return pval[pre[i >> 5] + __popc(w & (b - 1u))] * inv_t;
    }
    return ld<DT>(row, i) * inv_t;
  };

  const int64_t kk = p.top_k ? p.top_k[r] : 0;
  const float tp = p.top_p ? p.top_p[r] : 1.f;
  const bool sample_row = p.sample && p.do_sample && p.do_sample[r] != 0;
  const bool want_sum = sample_row || p.probs || p.logprobs || p.n_top > 0;
  const bool need_filter = want_sum || p.processed;  // a greedy token alone needs no filter
  const bool topk_on = need_filter && kk > 0 && kk < V;
  const bool topp_on = need_filter && tp < 1.0f;  // NaN or >= 1: off

  // ---- max: greedy token and softmax shift ---------------------------------------------------
  u64 best = 0;
  for (int i = tid; i < V; i += kThreads) {
    const u64 c = composite(proc(i), i);
    best = c > best ? c : best;
  }
  best = block_max_u64(best, sm);
  const float m = key2f((uint32_t)(best >> 32));
  const int top_i = composite_index(best);

  // ---- top-k, then top-p over the top-k survivors ---------------------------------------------
  Filter f{0u, 0x7FFFFFFF};
  if (topk_on) {
    auto e = [&](int i, uint32_t& k, u64& w) { k = f2key(proc(i)); w = 1; return true; };
    f = radix_select<false>(e, V, (u64)(kk - 1), -1.f, m, sm);
  }
  if (topp_on) {
    const Filter fk = f;
    auto e = [&](int i, uint32_t& k, u64& w) {
      const float x = proc(i);
      k = f2key(x);
      if (!fk.keep(k, i)) return false;
      w = mass_q(x, m);
      return true;
    };
    f = radix_select<true>(e, V, 0ull, tp > 0.f ? tp : 0.f, m, sm);
    // the top-p boundary is a position among the top-k survivors: when it falls in the run of equal
    // keys that top-k cut, the tokens top-k dropped from that run stay dropped
    if (f.key == fk.key && fk.imax < f.imax) f.imax = fk.imax;
  }

  // ---- sample: the survivors' sum of exp(x - m), exponential race ------------------------------
  int token = top_i;  // argmax(processed): the top element always survives
  if (want_sum) {
    const u64 seed = p.seeds ? p.seeds[r] : 0ull;
    const uint32_t pos = p.positions ? (uint32_t)p.positions[r] : 0u;
    float s = 0.f;
    u64 race = 0;
    for (int i = tid; i < V; i += kThreads) {
      const float x = proc(i);
      if (!f.keep(f2key(x), i)) continue;
      const float e = expm(x, m);
      s += e;
      if (sample_row) {  // argmax(probs / E) = argmax(exp(x - m) / E): the common 1 / sum drops out
        const float sc = e / exp_draw(philox_word(seed, pos, 0u, (uint32_t)i));
        const u64 c = composite(sc, i);
        race = c > race ? c : race;
      }
    }
    s = block_sum_f(s, sm);
    const float lse = logf(s);
    if (sample_row) token = composite_index(block_max_u64(race, sm));
    if (p.logprobs && tid == 0) p.logprobs[r] = (proc(token) - m) - lse;

    // ---- top-n of log_softmax(processed) ------------------------------------------------------
    if (p.n_top > 0) {
      auto e = [&](int i, uint32_t& k, u64& w) {
        const uint32_t k0 = f2key(proc(i));
        k = f.keep(k0, i) ? k0 : kKeyNegInf;
        w = 1;
        return true;
      };
      const Filter fn = radix_select<false>(e, V, (u64)(p.n_top - 1), -1.f, m, sm);
      gather_sort_top(e, V, p.n_top, fn, sm);
      if (tid == 0) {
        const int n = p.n_top;
        for (int a = 0; a < n; ++a) {
          const float x = key2f(sm.top_key[a]);
          p.top_lp[r * n + a] = x == -INFINITY ? -INFINITY : (x - m) - lse;
          p.top_tok[r * n + a] = sm.top_idx[a];
        }
      }
    }
    if (p.probs) {
      float* pr = p.probs + r * (int64_t)V;
      for (int i = tid; i < V; i += kThreads) {
        const float x = proc(i);
        pr[i] = f.keep(f2key(x), i) ? expm(x, m) / s : 0.f;
      }
    }
  }
  if (p.sample && tid == 0) p.next_tokens[r] = token;

  // ---- processed logits: the last pass that reads the row --------------------------------------
  if (p.processed) {
    __syncthreads();  // thread 0's reads of arbitrary tokens (logprob) are done: in place is safe
    void* out = reinterpret_cast<char*>(p.processed) + r * p.ld_out * elem_bytes<DT>();
    for (int i = tid; i < V; i += kThreads) {  // token i is read and written by the same thread
      const float x = proc(i);
      st<DT>(out, i, f.keep(f2key(x), i) ? x : -INFINITY);
    }
  }
}

int validate(const slm_sampling_args* a, bool sample) {
  if (!a || a->n_rows < 0) return SLM_ERR_INVALID_ARG;
  if (a->n_rows == 0) return SLM_OK;
  if (!a->logits) return SLM_ERR_INVALID_ARG;
  if (a->dtype != SLM_F16 && a->dtype != SLM_BF16 && a->dtype != SLM_F32) return SLM_ERR_UNSUPPORTED;
  if (a->vocab < 1 || a->logits_stride < a->vocab) return SLM_ERR_INVALID_ARG;
  if (a->vocab > kMaxVocab) return SLM_ERR_UNSUPPORTED;
  if (sample) {
    if (!a->next_tokens) return SLM_ERR_INVALID_ARG;
    if (a->n_top < 0 || a->n_top > SLM_SAMPLE_MAX_TOP || a->n_top > a->vocab) return SLM_ERR_INVALID_ARG;
    if (a->n_top > 0 && (!a->top_logprobs || !a->top_tokens)) return SLM_ERR_INVALID_ARG;
  } else if (!a->processed) {
    return SLM_ERR_INVALID_ARG;
  }
  if (a->processed && a->processed_stride < a->vocab) return SLM_ERR_INVALID_ARG;
  const bool fp = a->frequency_penalties || a->presence_penalties;
  if (fp || a->repetition_penalties) {
    if (!a->unique_ids || !a->unique_lens || a->max_unique < 0) return SLM_ERR_INVALID_ARG;
    if (fp && !a->unique_counts) return SLM_ERR_INVALID_ARG;
    if (a->max_unique > 0 && a->vocab > kMaxPenVocab) return SLM_ERR_UNSUPPORTED;
  }
  return SLM_OK;
}

bool has_penalties(const slm_sampling_args* a) {
  return (a->frequency_penalties || a->presence_penalties || a->repetition_penalties) && a->max_unique > 0;
}

// in place with penalties alone (the drop-in apply_*_penalty): only the penalised entries change
bool sparse_call(const slm_sampling_args* a, bool sample) {
  return !sample && a->processed == a->logits && a->processed_stride == a->logits_stride && !a->temperatures &&
         !a->top_k && !a->top_p;
}

size_t workspace_bytes(const slm_sampling_args* a) {
  if (!a || a->n_rows <= 0 || !has_penalties(a)) return 0;
  return ((size_t)a->n_rows * (size_t)a->max_unique * sizeof(float) + 255) & ~(size_t)255;
}

int launch(const slm_sampling_args* a, void* stream, bool sample) {
  const int rc = validate(a, sample);
  if (rc != SLM_OK || a->n_rows == 0) return rc;
  Params p{};
  p.logits = a->logits; p.ld_in = a->logits_stride; p.V = a->vocab; p.max_unique = a->max_unique;
  p.freq = a->frequency_penalties; p.pres = a->presence_penalties; p.rep = a->repetition_penalties;
  p.temp = a->temperatures; p.top_p = a->top_p; p.top_k = a->top_k;
  p.ids = a->unique_ids; p.counts = a->unique_counts; p.lens = a->unique_lens;
  p.processed = a->processed; p.ld_out = a->processed_stride;
  p.sample = sample ? 1 : 0;
  if (sample) {
    p.do_sample = a->do_sample; p.seeds = a->seeds; p.positions = a->positions;
    p.next_tokens = a->next_tokens; p.probs = a->probs; p.logprobs = a->logprobs;
    p.top_lp = a->top_logprobs; p.top_tok = a->top_tokens; p.n_top = a->n_top;
  }
  p.has_pen = has_penalties(a) ? 1 : 0;
  p.sparse = sparse_call(a, sample) ? 1 : 0;
  if (p.sparse && !p.has_pen) return SLM_OK;  // nothing changes
  size_t lds = 0;
  if (p.has_pen && !p.sparse) {
    const size_t need = workspace_bytes(a);
    if (!a->workspace || a->workspace_bytes < need) return SLM_ERR_WORKSPACE;
    p.ws = reinterpret_cast<float*>(a->workspace);
    lds = 2 * (size_t)((a->vocab + 31) / 32) * sizeof(uint32_t);
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hip_clear_error();
  auto go = [&](auto kfn) {
    if (lds > 48 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds);
    hipLaunchKernelGGL(kfn, dim3(a->n_rows), dim3(kThreads), lds, s, p);
  };
  switch (a->dtype) {
    case SLM_F16: go(sample_kernel<SLM_F16>); break;
    case SLM_BF16: go(sample_kernel<SLM_BF16>); break;
    default: go(sample_kernel<SLM_F32>); break;
  }
  return hip_check_launch();
}

}  // namespace
}  // namespace slm

extern "C" {

SLM_API size_t slm_sample_workspace_bytes(const slm_sampling_args* a) { return slm::workspace_bytes(a); }

SLM_API int slm_sample(const slm_sampling_args* a, void* stream) { return slm::launch(a, stream, true); }

SLM_API int slm_logits_process(const slm_sampling_args* a, void* stream) { return slm::launch(a, stream, false); }

}  // extern "C"
