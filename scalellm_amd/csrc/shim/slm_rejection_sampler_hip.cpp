// slm_rejection_sampler_hip.cpp -- see slm_rejection_sampler_hip.h.  Host code only: tensors are unpacked into
// slm_rejection_args and handed to slm_rejection_sample on torch's current HIP stream.
#include "slm_rejection_sampler_hip.h"

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/hip/HIPGraphsC10Utils.h>

#include <mutex>
#include <unordered_map>
#include <vector>

#include "slm_hip.h"

namespace {

// the per-row records: one growable buffer per device, never released (captured graphs keep its address),
// growth refused during capture
std::mutex g_mu;
std::unordered_map<int, torch::Tensor> g_ws;
std::vector<torch::Tensor> g_retired;

torch::Tensor workspace(const torch::Tensor& like, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto& ws = g_ws[like.device().index()];
  if (!ws.defined() || static_cast<size_t>(ws.nbytes()) < bytes) {
    TORCH_CHECK(c10::hip::currentStreamCaptureStatusMayInitCtx() == c10::hip::CaptureStatus::None,
                "slm rejection sampler: the workspace must be sized before graph capture (run once eagerly)");
    if (ws.defined()) g_retired.push_back(ws);
    const int64_t n = std::max<int64_t>(static_cast<int64_t>(bytes), ws.defined() ? 2 * ws.numel() : 0);
    ws = torch::empty({std::max<int64_t>(n, 1 << 16)}, like.options().dtype(torch::kUInt8));
  }
  return ws;
}

// a [count] contiguous tensor of `dtype` (kept alive in `keep`), or NULL
const void* flat(const torch::Tensor& t, int64_t count, torch::ScalarType dtype, const char* what,
                 std::vector<torch::Tensor>& keep) {
  if (!t.defined()) return nullptr;
  TORCH_CHECK(t.is_cuda(), "slm rejection sampler: ", what, " must be a GPU tensor");
  auto v = t.reshape({-1});
  TORCH_CHECK(v.numel() == count, "slm rejection sampler: ", what, " has ", v.numel(), " values, expected ", count);
  if (v.scalar_type() != dtype || !v.is_contiguous()) v = v.to(dtype).contiguous();
  keep.push_back(v);
  return v.data_ptr();
}

void rows3(const torch::Tensor& t, int64_t n, int64_t rows, int64_t V, const char* what, int64_t* ld_s, int64_t* ld_r) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 3 && t.size(0) == n && t.size(1) >= rows && t.size(2) == V && t.stride(2) == 1,
              "slm rejection sampler: ", what, " must be a GPU [n_seqs, ", rows, ", vocab] tensor with contiguous rows");
  *ld_s = t.stride(0);
  *ld_r = t.stride(1);
}

torch::Tensor mask_after(const torch::Tensor& tokens, const torch::Tensor& accepted_lens) {
  auto keep = torch::arange(tokens.size(1), tokens.options()).unsqueeze(0) < accepted_lens.unsqueeze(1);
  return torch::where(keep, tokens, torch::full_like(tokens, -1));
}

}  // namespace

namespace slm {

SampleOutput rejection_sample(const torch::Tensor& draft_token_ids, const torch::Tensor& draft_probs,
                              const torch::Tensor& target, const torch::Tensor& bonus_token_ids, bool target_is_probs,
                              bool mask_out_rejected_tokens, const torch::Tensor& do_sample,
                              const torch::Tensor& seeds, const torch::Tensor& positions,
                              const torch::Tensor& uniform, bool logprobs, int64_t max_top_logprobs,
                              const SampleOutput* out) {
  TORCH_CHECK(draft_token_ids.dim() == 2, "slm rejection sampler: draft_token_ids must be [n_seqs, k]");
  TORCH_CHECK(target.dim() == 3, "slm rejection sampler: target must be [n_seqs, rows, vocab]");
  const int64_t n = draft_token_ids.size(0), k = draft_token_ids.size(1), V = target.size(2);
  std::vector<torch::Tensor> keep;
  slm_rejection_args a{};
  a.n_seqs = static_cast<int32_t>(n);
  a.k = static_cast<int32_t>(k);
  a.vocab = static_cast<int32_t>(V);
  a.target_is_probs = target_is_probs ? 1 : 0;
  a.mask_out_rejected = mask_out_rejected_tokens ? 1 : 0;
  if (target.scalar_type() == torch::kBFloat16) a.dtype = SLM_BF16;
  else if (target.scalar_type() == torch::kHalf) a.dtype = SLM_F16;
  else if (target.scalar_type() == torch::kFloat) a.dtype = SLM_F32;
  else TORCH_CHECK(false, "slm rejection sampler: fp16 / bf16 / fp32 target only, got ", target.scalar_type());
  a.target = target.data_ptr();
  rows3(target, n, target_is_probs ? k : k + 1, V, "target", &a.target_seq_stride, &a.target_row_stride);
  if (draft_probs.defined()) {
    TORCH_CHECK(draft_probs.scalar_type() == torch::kFloat, "slm rejection sampler: draft_probs must be fp32");
    a.draft_probs = draft_probs.data_ptr<float>();
    rows3(draft_probs, n, k, V, "draft_probs", &a.draft_seq_stride, &a.draft_row_stride);
  }
  a.draft_token_ids = static_cast<const int32_t*>(flat(draft_token_ids, n * k, torch::kInt, "draft_token_ids", keep));
  a.bonus_token_ids = static_cast<const int32_t*>(flat(bonus_token_ids, n, torch::kInt, "bonus_token_ids", keep));
  a.do_sample = static_cast<const uint8_t*>(flat(do_sample, n, torch::kBool, "do_sample", keep));
  a.seeds = static_cast<const uint64_t*>(flat(seeds, n, torch::kLong, "seeds", keep));
  a.positions = static_cast<const int32_t*>(flat(positions, n, torch::kInt, "positions", keep));
  a.uniform = static_cast<const float*>(flat(uniform, n * k, torch::kFloat, "uniform", keep));
  SampleOutput o;
  if (out) {
    o = *out;
  } else {
    const auto f = target.options().dtype(torch::kFloat), i = target.options().dtype(torch::kInt);
    o.next_tokens = torch::empty({n, k + 1}, i);
    o.accepted_lens = torch::empty({n}, i);
    if (logprobs) {
      o.logprobs = torch::empty({n, k + 1}, f);
      if (max_top_logprobs > 0) {
        o.top_logprobs = torch::empty({n, k + 1, max_top_logprobs}, f);
        o.top_tokens = torch::empty({n, k + 1, max_top_logprobs}, i);
      }
    }
  }
  auto check_out = [&](const torch::Tensor& t, int64_t count, torch::ScalarType dt, const char* what) {
    TORCH_CHECK(t.scalar_type() == dt && t.is_contiguous() && t.numel() == count, "slm rejection sampler: ", what,
                " must be contiguous ", dt, " with ", count, " entries");
  };
  TORCH_CHECK(o.next_tokens.defined(), "slm rejection sampler: next_tokens is required");
  check_out(o.next_tokens, n * (k + 1), torch::kInt, "next_tokens");
  a.next_tokens = o.next_tokens.data_ptr<int32_t>();
  if (o.accepted_lens.defined()) {
    check_out(o.accepted_lens, n, torch::kInt, "accepted_lens");
    a.accepted_lens = o.accepted_lens.data_ptr<int32_t>();
  }
  if (o.logprobs.defined()) {
    check_out(o.logprobs, n * (k + 1), torch::kFloat, "logprobs");
    a.logprobs = o.logprobs.data_ptr<float>();
  }
  if (o.top_tokens.defined()) {
    const int64_t nt = o.top_tokens.size(-1);
    TORCH_CHECK(o.top_logprobs.defined(), "slm rejection sampler: top_tokens without top_logprobs");
    check_out(o.top_tokens, n * (k + 1) * nt, torch::kInt, "top_tokens");
    check_out(o.top_logprobs, n * (k + 1) * nt, torch::kFloat, "top_logprobs");
    a.top_logprobs = o.top_logprobs.data_ptr<float>();
    a.top_tokens = o.top_tokens.data_ptr<int32_t>();
    a.n_top = static_cast<int32_t>(nt);
  }
  const size_t need = slm_rejection_sample_workspace_bytes(&a);
  if (need) {
    auto ws = workspace(target, need);
    keep.push_back(ws);
    a.workspace = ws.data_ptr();
    a.workspace_bytes = static_cast<size_t>(ws.nbytes());
  }
  void* stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(target.device().index()).stream();
  const int rc = slm_rejection_sample(&a, stream);
  TORCH_CHECK(rc == SLM_OK, "slm_rejection_sample failed: ", slm_status_string(rc), " (", rc, ")",
              rc == SLM_ERR_LAUNCH ? slm_last_hip_error() : "");
  return o;
}

RejectionSampler::RejectionSampler(const torch::Tensor& do_sample, bool logprobs, int64_t max_top_logprobs,
                                   const torch::Tensor& seeds, const torch::Tensor& positions)
    : logprobs_(logprobs), max_top_logprobs_(max_top_logprobs), do_sample_(do_sample), seeds_(seeds),
      positions_(positions) {
  TORCH_CHECK(max_top_logprobs >= 0 && max_top_logprobs <= SLM_SAMPLE_MAX_TOP,
              "slm rejection sampler: max_top_logprobs outside 0..", SLM_SAMPLE_MAX_TOP);
}

SampleOutput RejectionSampler::forward(const torch::Tensor& draft_token_ids, const torch::Tensor& draft_probs,
                                       const torch::Tensor& target_logits, const torch::Tensor& bonus_token_ids,
                                       bool mask_out_rejected_tokens) const {
  return rejection_sample(draft_token_ids, draft_probs, target_logits, bonus_token_ids, false,
                          mask_out_rejected_tokens, do_sample_, seeds_, positions_, torch::Tensor(), logprobs_,
                          logprobs_ ? max_top_logprobs_ : 0);
}

torch::Tensor RejectionSampler::build_accepted_mask(const torch::Tensor& accepted) {
  const int64_t n = accepted.size(0), k = accepted.size(1);
  auto rejected = torch::cat({accepted.to(torch::kBool).logical_not(),
                              torch::ones({n, 1}, accepted.options().dtype(torch::kBool))}, /*dim=*/1);
  auto first = rejected.to(torch::kInt).argmax(/*dim=*/1, /*keepdim=*/true);  // the first rejected row
  return torch::arange(k + 1, accepted.options().dtype(torch::kLong)).unsqueeze(0) <= first;
}

std::tuple<torch::Tensor, torch::Tensor> RejectionSampler::random_sample(
    const torch::Tensor& draft_token_ids, const torch::Tensor& draft_probs, const torch::Tensor& target_probs,
    const torch::Tensor& uniform_rand, const torch::Tensor& bonus_token_ids, bool mask_out_rejected_tokens,
    const torch::Tensor& seeds, const torch::Tensor& positions) {
  auto all = torch::ones({draft_token_ids.size(0)}, draft_token_ids.options().dtype(torch::kBool));
  auto o = rejection_sample(draft_token_ids, draft_probs, target_probs, bonus_token_ids, true, false, all, seeds,
                            positions, uniform_rand, false, 0);
  return {o.next_tokens, mask_out_rejected_tokens ? mask_after(o.next_tokens, o.accepted_lens) : torch::Tensor()};
}

std::tuple<torch::Tensor, torch::Tensor> RejectionSampler::greedy_sample(const torch::Tensor& draft_token_ids,
                                                                        const torch::Tensor& target_probs,
                                                                        const torch::Tensor& bonus_token_ids,
                                                                        bool mask_out_rejected_tokens) {
  auto o = rejection_sample(draft_token_ids, torch::Tensor(), target_probs, bonus_token_ids, true, false,
                            torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor(), false, 0);
  return {o.next_tokens, mask_out_rejected_tokens ? mask_after(o.next_tokens, o.accepted_lens) : torch::Tensor()};
}

}  // namespace slm
