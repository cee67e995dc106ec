// slm_rejection_sampler_hip.h -- validation of speculative drafts at the libtorch boundary, on top of the C
// ABI's section 9 (include/slm_hip.h: slm_rejection_sample, csrc/rejection.hip).
//
//   slm::RejectionSampler  the reference's llm::RejectionSampler (src/speculative/rejection_sampler.h) with the
//                          same methods and parameter lists; seeds and positions are optional trailing
//                          arguments, as in slm::Sampler.  Token ids are int32, as slm::SampleOutput holds
//                          them (the reference returns int64).  Nothing synchronises with the host: the
//                          constructor does not read do_sample, so forward() can be captured in a graph.
// Python mirror: scalellm_amd/speculative.py (same kernel, same arguments: bit-identical results).
#pragma once
#include <torch/torch.h>

#include <tuple>
#include <utility>

#include "slm_sampling_hip.h"

namespace slm {

// One slm_rejection_sample call.  target: [n, k + 1, V] logits (f16 / bf16 / fp32) or, with target_is_probs,
// [n, k, V] fp32 probabilities; draft_probs [n, k, V] fp32 (undefined: every sequence greedy); strided rows
// are read in place.  `out` (optional): the output tensors to fill (a captured step's static buffers).
SampleOutput rejection_sample(const torch::Tensor& draft_token_ids, const torch::Tensor& draft_probs,
                              const torch::Tensor& target, const torch::Tensor& bonus_token_ids, bool target_is_probs,
                              bool mask_out_rejected_tokens, const torch::Tensor& do_sample,
                              const torch::Tensor& seeds, const torch::Tensor& positions,
                              const torch::Tensor& uniform, bool logprobs, int64_t max_top_logprobs,
                              const SampleOutput* out = nullptr);

class RejectionSampler final {
 public:
  RejectionSampler(const torch::Tensor& do_sample, bool logprobs, int64_t max_top_logprobs,
                   const torch::Tensor& seeds = torch::Tensor(), const torch::Tensor& positions = torch::Tensor());

  template <typename... Args>
  auto operator()(Args&&... args) const {
    return this->forward(::std::forward<Args>(args)...);
  }

  // draft_token_ids [n, k]; draft_probs [n, k, V]; target_logits [n, k + 1, V]; bonus_token_ids [n, 1].
  // next_tokens [n, k + 1] int32 (-1 after the first rejected row when masked); accepted_lens [n];
  // logprobs / top logprobs of every target row at the unmasked tokens.
  SampleOutput forward(const torch::Tensor& draft_token_ids, const torch::Tensor& draft_probs,
                       const torch::Tensor& target_logits, const torch::Tensor& bonus_token_ids,
                       bool mask_out_rejected_tokens = false) const;

  // [n, k] accepted -> [n, k + 1] bool: true up to and including the first rejected row
  static torch::Tensor build_accepted_mask(const torch::Tensor& accepted);

  // on fp32 target probabilities [n, k, V]: (tokens, masked tokens -- undefined without masking)
  static std::tuple<torch::Tensor, torch::Tensor> random_sample(
      const torch::Tensor& draft_token_ids, const torch::Tensor& draft_probs, const torch::Tensor& target_probs,
      const torch::Tensor& uniform_rand, const torch::Tensor& bonus_token_ids, bool mask_out_rejected_tokens,
      const torch::Tensor& seeds = torch::Tensor(), const torch::Tensor& positions = torch::Tensor());

  static std::tuple<torch::Tensor, torch::Tensor> greedy_sample(const torch::Tensor& draft_token_ids,
                                                                const torch::Tensor& target_probs,
                                                                const torch::Tensor& bonus_token_ids,
                                                                bool mask_out_rejected_tokens);

 private:
  bool logprobs_ = false;
  int64_t max_top_logprobs_ = 0;
  torch::Tensor do_sample_, seeds_, positions_;
};

}  // namespace slm
