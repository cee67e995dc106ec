// slm_sampling_hip.h -- logits processing and sampling at the libtorch boundary, on top of the C ABI's
// section 8 (include/slm_hip.h: slm_sample / slm_logits_process, csrc/sampling.hip).
//
//   llm::kernel::apply_temperature_penalty / apply_repetition_penalty / apply_frequency_presence_penalty /
//   invoke_softmax   the reference's signatures verbatim (src/kernels/sampling/sampling_kernels.h:7-28), so
//                    its own LogitsProcessor (src/sampling/logits_processor.h) links against HIP unchanged.
//                    invoke_topk_sampling is not offered: it takes a curandState_t* and nothing in the
//                    reference calls it (the sampler is torch code, src/sampling/sampler.cpp).
//   slm::SamplingParameters / LogitsProcessor / Sampler / SampleOutput
//                    the reference's objects (parameters.h, logits_processor.h, sampler.h) over ONE launch,
//                    plus per-row seeds; slm::sample runs processing and sampling fused.
// Python mirror: scalellm_amd/sampling.py (same kernel, same arguments: bit-identical results).
#pragma once
#include <torch/torch.h>

#include <memory>

namespace llm {
namespace kernel {

void apply_temperature_penalty(torch::Tensor& logits, const torch::Tensor& temperatures);

void apply_repetition_penalty(torch::Tensor& logits, const torch::Tensor& token_ids,
                              const torch::Tensor& token_ids_lens, const torch::Tensor& penalities);

void apply_frequency_presence_penalty(torch::Tensor& logits, const torch::Tensor& token_ids,
                                      const torch::Tensor& token_counts, const torch::Tensor& token_ids_lens,
                                      const torch::Tensor& frequency_penalties,
                                      const torch::Tensor& presence_penalties);

// softmax over the last dim, in place (fp32 arithmetic, rounded once to the logits dtype)
void invoke_softmax(torch::Tensor& logits);

}  // namespace kernel
}  // namespace llm

namespace slm {

// parameters.h:33-119, one row per sampled sequence; an undefined tensor is neutral for every row.
// Float parameters are converted to fp32, ids to int64, counts / lens to int32, do_sample to bool.
struct SamplingParameters {
  torch::Tensor frequency_penalties, presence_penalties, repetition_penalties, temperatures, top_p;
  torch::Tensor top_k;                   // int64
  torch::Tensor unique_token_ids;        // [n, max_unique] int64
  torch::Tensor unique_token_counts;     // [n, max_unique] int32
  torch::Tensor unique_token_ids_lens;   // [n] int32
  torch::Tensor do_sample;               // [n] bool
  torch::Tensor seeds;                   // [n] int64 (the uint64 seed's bits)
  bool logprobs = false;
  int64_t max_top_logprobs = 0;
  SamplingParameters narrow(int64_t n) const;  // rows [0, n) as views
};

// parameters.h:121-135 (next_tokens int32).  accepted_lens: the rejection sampler's addition (first rejected
// row + 1 per sequence; undefined elsewhere).
struct SampleOutput {
  torch::Tensor next_tokens, probs, logprobs, top_logprobs, top_tokens;
  torch::Tensor accepted_lens;
};

// LogitsProcessor + Sampler in one launch.  positions[r]: position of row r's last input token (the RNG
// counter).  `out` (optional): the output tensors to fill (a captured step's static buffers); otherwise
// they are allocated (probs only with want_probs).
SampleOutput sample(const torch::Tensor& logits, const SamplingParameters& params, const torch::Tensor& positions,
                    const SampleOutput* out = nullptr, bool want_probs = false);

// LogitsProcessor::create (logits_processor.h:89-90): penalties, temperature, top-k / top-p in one launch,
// in place on `logits` (returned)
class LogitsProcessor {
 public:
  explicit LogitsProcessor(const SamplingParameters& params) : params_(params) {}
  static std::unique_ptr<LogitsProcessor> create(const SamplingParameters& params);
  torch::Tensor forward(const torch::Tensor& logits, const torch::Tensor& unique_token_ids,
                        const torch::Tensor& unique_token_counts, const torch::Tensor& unique_token_lens) const;

 private:
  SamplingParameters params_;
};

// Sampler (sampler.h, sampler.cpp:9-70) on processed logits; seeds / positions drive the RNG
class Sampler {
 public:
  Sampler(const torch::Tensor& do_sample, bool logprobs, int64_t max_top_logprobs,
          const torch::Tensor& seeds = torch::Tensor(), const torch::Tensor& positions = torch::Tensor());
  SampleOutput forward(const torch::Tensor& logits) const;

 private:
  torch::Tensor do_sample_, seeds_, positions_;
  bool logprobs_;
  int64_t max_top_logprobs_;
};

}  // namespace slm
