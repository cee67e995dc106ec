// slm_sampling_hip.cpp -- see slm_sampling_hip.h.  Host code only: tensors are unpacked into
// slm_sampling_args and handed to slm_sample / slm_logits_process on torch's current HIP stream.
#include "slm_sampling_hip.h"

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/hip/HIPGraphsC10Utils.h>

#include <mutex>
#include <unordered_map>
#include <vector>

#include "slm_hip.h"

namespace {

void check(int rc, const char* what) {
  TORCH_CHECK(rc == SLM_OK, what, " failed: ", slm_status_string(rc), " (", rc, ")",
              rc == SLM_ERR_LAUNCH ? slm_last_hip_error() : "");
}

int logits_dtype(const torch::Tensor& t) {
  if (t.scalar_type() == torch::kBFloat16) return SLM_BF16;
  if (t.scalar_type() == torch::kHalf) return SLM_F16;
  if (t.scalar_type() == torch::kFloat) return SLM_F32;
  TORCH_CHECK(false, "slm sampling: fp16 / bf16 / fp32 logits only, got ", t.scalar_type());
  return -1;
}

// the penalised-value scratch: one growable buffer per device, never released (captured graphs keep
// its address), growth refused during capture
std::mutex g_mu;
std::unordered_map<int, torch::Tensor> g_ws;
std::vector<torch::Tensor> g_retired;

torch::Tensor workspace(const torch::Tensor& like, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto& ws = g_ws[like.device().index()];
  if (!ws.defined() || static_cast<size_t>(ws.nbytes()) < bytes) {
    TORCH_CHECK(c10::hip::currentStreamCaptureStatusMayInitCtx() == c10::hip::CaptureStatus::None,
                "slm sampling: the workspace must be sized before graph capture (run the step once eagerly)");
    if (ws.defined()) g_retired.push_back(ws);
    const int64_t n = std::max<int64_t>(static_cast<int64_t>(bytes), ws.defined() ? 2 * ws.numel() : 0);
    ws = torch::empty({std::max<int64_t>(n, 1 << 20)}, like.options().dtype(torch::kUInt8));
  }
  return ws;
}

// a per-row parameter as a contiguous [n] tensor of `dtype` (kept alive in `keep`), or NULL
const void* rows(const torch::Tensor& t, int64_t n, torch::ScalarType dtype, const char* what,
                 std::vector<torch::Tensor>& keep) {
  if (!t.defined()) return nullptr;
  TORCH_CHECK(t.is_cuda(), "slm sampling: ", what, " must be a GPU tensor");
  auto v = t.reshape({-1});
  TORCH_CHECK(v.numel() == n, "slm sampling: ", what, " has ", v.numel(), " values for ", n, " rows");
  if (v.scalar_type() != dtype || !v.is_contiguous()) v = v.to(dtype).contiguous();
  keep.push_back(v);
  return v.data_ptr();
}

struct Call {
  slm_sampling_args a{};
  std::vector<torch::Tensor> keep;
};

Call make_call(const torch::Tensor& logits, const slm::SamplingParameters& p, bool penalties) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1,
              "slm sampling: logits must be a GPU [n_rows, vocab] tensor with contiguous rows");
  Call c;
  auto& a = c.a;
  const int64_t n = logits.size(0);
  a.logits = logits.data_ptr();
  a.logits_stride = logits.stride(0);
  a.dtype = logits_dtype(logits);
  a.n_rows = static_cast<int32_t>(n);
  a.vocab = static_cast<int32_t>(logits.size(1));
  a.temperatures = static_cast<const float*>(rows(p.temperatures, n, torch::kFloat, "temperatures", c.keep));
  a.top_p = static_cast<const float*>(rows(p.top_p, n, torch::kFloat, "top_p", c.keep));
  a.top_k = static_cast<const int64_t*>(rows(p.top_k, n, torch::kLong, "top_k", c.keep));
  if (penalties && p.unique_token_ids.defined()) {
    a.frequency_penalties = static_cast<const float*>(rows(p.frequency_penalties, n, torch::kFloat, "frequency_penalties", c.keep));
    a.presence_penalties = static_cast<const float*>(rows(p.presence_penalties, n, torch::kFloat, "presence_penalties", c.keep));
    a.repetition_penalties = static_cast<const float*>(rows(p.repetition_penalties, n, torch::kFloat, "repetition_penalties", c.keep));
    auto ids = p.unique_token_ids.reshape({n, -1});
    if (ids.scalar_type() != torch::kLong || !ids.is_contiguous()) ids = ids.to(torch::kLong).contiguous();
    c.keep.push_back(ids);
    a.unique_ids = ids.data_ptr<int64_t>();
    a.max_unique = static_cast<int32_t>(ids.size(1));
    if (p.unique_token_counts.defined()) {
      auto cnt = p.unique_token_counts.reshape({n, -1});
      TORCH_CHECK(cnt.size(1) == ids.size(1), "slm sampling: unique_token_counts / unique_token_ids differ");
      if (cnt.scalar_type() != torch::kInt || !cnt.is_contiguous()) cnt = cnt.to(torch::kInt).contiguous();
      c.keep.push_back(cnt);
      a.unique_counts = cnt.data_ptr<int32_t>();
    }
    a.unique_lens = static_cast<const int32_t*>(rows(p.unique_token_ids_lens, n, torch::kInt, "unique_token_ids_lens", c.keep));
  }
  return c;
}

void launch(Call& c, const torch::Tensor& logits, bool sample) {
  const size_t need = slm_sample_workspace_bytes(&c.a);
  if (need) {
    auto ws = workspace(logits, need);
    c.keep.push_back(ws);
    c.a.workspace = ws.data_ptr();
    c.a.workspace_bytes = static_cast<size_t>(ws.nbytes());
  }
  void* stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(logits.device().index()).stream();
  if (sample) check(slm_sample(&c.a, stream), "slm_sample");
  else check(slm_logits_process(&c.a, stream), "slm_logits_process");
}

void process_in_place(torch::Tensor& logits, const slm::SamplingParameters& p) {
  auto c = make_call(logits, p, true);
  c.a.processed = logits.data_ptr();
  c.a.processed_stride = logits.stride(0);
  launch(c, logits, false);
}

}  // namespace

namespace llm {
namespace kernel {

void apply_temperature_penalty(torch::Tensor& logits, const torch::Tensor& temperatures) {
  slm::SamplingParameters p;
  p.temperatures = temperatures;
  process_in_place(logits, p);
}

void apply_repetition_penalty(torch::Tensor& logits, const torch::Tensor& token_ids,
                              const torch::Tensor& token_ids_lens, const torch::Tensor& penalities) {
  slm::SamplingParameters p;
  p.unique_token_ids = token_ids;
  p.unique_token_ids_lens = token_ids_lens;
  p.repetition_penalties = penalities;
  process_in_place(logits, p);
}

void apply_frequency_presence_penalty(torch::Tensor& logits, const torch::Tensor& token_ids,
                                      const torch::Tensor& token_counts, const torch::Tensor& token_ids_lens,
                                      const torch::Tensor& frequency_penalties,
                                      const torch::Tensor& presence_penalties) {
  slm::SamplingParameters p;
  p.unique_token_ids = token_ids;
  p.unique_token_counts = token_counts;
  p.unique_token_ids_lens = token_ids_lens;
  p.frequency_penalties = frequency_penalties;
  p.presence_penalties = presence_penalties;
  process_in_place(logits, p);
}

void invoke_softmax(torch::Tensor& logits) {
  auto c = make_call(logits, slm::SamplingParameters(), false);
  const int64_t n = logits.size(0);
  auto tok = torch::empty({n}, logits.options().dtype(torch::kInt));
  auto probs = torch::empty({n, logits.size(1)}, logits.options().dtype(torch::kFloat));
  c.a.next_tokens = tok.data_ptr<int32_t>();
  c.a.probs = probs.data_ptr<float>();
  launch(c, logits, true);
  logits.copy_(probs);
}

}  // namespace kernel
}  // namespace llm

namespace slm {

SamplingParameters SamplingParameters::narrow(int64_t n) const {
  SamplingParameters o = *this;
  for (torch::Tensor* t : {&o.frequency_penalties, &o.presence_penalties, &o.repetition_penalties, &o.temperatures,
                           &o.top_p, &o.top_k, &o.unique_token_ids, &o.unique_token_counts, &o.unique_token_ids_lens,
                           &o.do_sample, &o.seeds})
    if (t->defined()) *t = t->narrow(0, 0, n);
  return o;
}

SampleOutput sample(const torch::Tensor& logits, const SamplingParameters& p, const torch::Tensor& positions,
                    const SampleOutput* out, bool want_probs) {
  auto c = make_call(logits, p, true);
  const int64_t n = logits.size(0), V = logits.size(1);
  auto& a = c.a;
  a.do_sample = static_cast<const uint8_t*>(rows(p.do_sample, n, torch::kBool, "do_sample", c.keep));
  a.seeds = static_cast<const uint64_t*>(rows(p.seeds, n, torch::kLong, "seeds", c.keep));
  a.positions = static_cast<const int32_t*>(rows(positions, n, torch::kInt, "positions", c.keep));
  SampleOutput o;
  if (out) {
    o = *out;
  } else {
    const auto f = logits.options().dtype(torch::kFloat), i = logits.options().dtype(torch::kInt);
    o.next_tokens = torch::empty({n}, i);
    if (want_probs) o.probs = torch::empty({n, V}, f);
    if (p.logprobs) {
      o.logprobs = torch::empty({n}, f);
      if (p.max_top_logprobs > 0) {
        o.top_logprobs = torch::empty({n, p.max_top_logprobs}, f);
        o.top_tokens = torch::empty({n, p.max_top_logprobs}, i);
      }
    }
  }
  TORCH_CHECK(o.next_tokens.defined() && o.next_tokens.scalar_type() == torch::kInt && o.next_tokens.is_contiguous() &&
                  o.next_tokens.numel() == n, "slm::sample: next_tokens must be contiguous int32 [n_rows]");
  a.next_tokens = o.next_tokens.data_ptr<int32_t>();
  if (o.probs.defined()) {
    TORCH_CHECK(o.probs.scalar_type() == torch::kFloat && o.probs.is_contiguous() && o.probs.size(0) == n &&
                    o.probs.size(1) == V, "slm::sample: probs must be contiguous fp32 [n_rows, vocab]");
    a.probs = o.probs.data_ptr<float>();
  }
  if (o.logprobs.defined()) {
    TORCH_CHECK(o.logprobs.scalar_type() == torch::kFloat && o.logprobs.is_contiguous() && o.logprobs.numel() == n,
                "slm::sample: logprobs must be contiguous fp32 [n_rows]");
    a.logprobs = o.logprobs.data_ptr<float>();
  }
  if (o.top_tokens.defined()) {
    TORCH_CHECK(o.top_logprobs.defined() && o.top_tokens.is_contiguous() && o.top_logprobs.is_contiguous() &&
                    o.top_tokens.scalar_type() == torch::kInt && o.top_logprobs.scalar_type() == torch::kFloat &&
                    o.top_tokens.sizes() == o.top_logprobs.sizes() && o.top_tokens.size(0) == n,
                "slm::sample: top_logprobs (fp32) / top_tokens (int32) must be contiguous [n_rows, n_top]");
    a.top_logprobs = o.top_logprobs.data_ptr<float>();
    a.top_tokens = o.top_tokens.data_ptr<int32_t>();
    a.n_top = static_cast<int32_t>(o.top_tokens.size(1));
  }
  launch(c, logits, true);
  return o;
}

std::unique_ptr<LogitsProcessor> LogitsProcessor::create(const SamplingParameters& params) {
  return std::make_unique<LogitsProcessor>(params);
}

torch::Tensor LogitsProcessor::forward(const torch::Tensor& logits, const torch::Tensor& unique_token_ids,
                                       const torch::Tensor& unique_token_counts,
                                       const torch::Tensor& unique_token_lens) const {
  SamplingParameters p = params_;
  p.unique_token_ids = unique_token_ids;
  p.unique_token_counts = unique_token_counts;
  p.unique_token_ids_lens = unique_token_lens;
  torch::Tensor x = logits;
  process_in_place(x, p);
  return x;
}

Sampler::Sampler(const torch::Tensor& do_sample, bool logprobs, int64_t max_top_logprobs, const torch::Tensor& seeds,
                 const torch::Tensor& positions)
    : do_sample_(do_sample), seeds_(seeds), positions_(positions), logprobs_(logprobs),
      max_top_logprobs_(max_top_logprobs) {}

SampleOutput Sampler::forward(const torch::Tensor& logits) const {
  SamplingParameters p;
  p.do_sample = do_sample_;
  p.seeds = seeds_;
  p.logprobs = logprobs_;
  p.max_top_logprobs = max_top_logprobs_;
  return sample(logits, p, positions_, nullptr, /*want_probs=*/true);  // SampleOutput::probs, as sampler.cpp:28
}

}  // namespace slm
