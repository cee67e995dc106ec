// slm_mxfp4_linear_hip.cpp -- see slm_mxfp4_linear_hip.h.  Host code only.
#include "slm_mxfp4_linear_hip.h"

#include <algorithm>

namespace slm {

torch::Tensor Mxfp4LinearHipBase::bytes_of(const StateDict& sd, const std::string& name, int64_t cols) {
  auto t = sd.get_tensor(name);
  if (!t.defined()) return t;
  const auto st = t.scalar_type();
  // a scale may also come as float8_e8m0fnu, a weight as float4_e2m1fn_x2; the other's typed dtype means swapped keys
  const bool is_scale = name.size() >= 5 && name.compare(name.size() - 5, 5, "scale") == 0;
  const auto typed = is_scale ? c10::ScalarType::Float8_e8m0fnu : c10::ScalarType::Float4_e2m1fn_x2;
  TORCH_CHECK(st == torch::kUInt8 || st == typed, "mxfp4 linear: ", sd.prefix() + name, " must be uint8 bytes (or ",
              typed, "), not ", st, " (nothing is quantised on load)");
  if (st != torch::kUInt8) t = t.view(torch::kUInt8);
  if (t.dim() == 3) {  // the blocked form [N, K / 32, 16]
    TORCH_CHECK(t.size(2) == 16, sd.prefix() + name, ": the blocked form is [N, K/32, 16], not ", t.sizes());
    t = t.reshape({t.size(0), -1});
  }
  TORCH_CHECK(t.dim() == 2 && t.size(1) == cols, sd.prefix() + name, " size mismatch: ", t.sizes(), " for ", cols,
              " bytes per row");
  return t;
}

torch::Tensor Mxfp4LinearHipBase::shard(const torch::Tensor& t, int64_t dim, const std::string& what) const {
  const int world = parallel_args_.world_size();
  if (world <= 1) return t.to(options_.device());
  TORCH_CHECK(t.size(dim) % world == 0, "can't divide ", what, " evenly on dim ", dim, " with world_size ", world);
  return t.chunk(world, dim)[parallel_args_.rank()].to(options_.device());
}

void Mxfp4LinearHipBase::load_pair(const StateDict& sd, int64_t in_features, int64_t dim) {
  const auto w = bytes_of(sd, "weight", in_features / 2);
  if (w.defined()) {
    TORCH_CHECK(!weight_is_loaded_, "weight ", sd.prefix() + "weight", " is loaded twice");
    weight_ = shard(w, dim, "weight").contiguous();
    weight_is_loaded_ = true;
  }
  const auto s = bytes_of(sd, "weight_scale", in_features / 32);
  if (s.defined()) {
    TORCH_CHECK(!scale_is_loaded_, "weight ", sd.prefix() + "weight_scale", " is loaded twice");
    weight_scale_ = shard(s, dim, "weight_scale").contiguous();
    scale_is_loaded_ = true;
  }
}

void Mxfp4LinearHipBase::verify_loaded_weights(const std::string& prefix) const {
  TORCH_CHECK(weight_is_loaded_, "weight is not loaded for ", prefix + "weight");
  TORCH_CHECK(!has_bias_ || bias_is_loaded_, "bias is not loaded for ", prefix + "bias");
  TORCH_CHECK(scale_is_loaded_, "weight_scale is not loaded for ", prefix + "weight_scale");
  TORCH_CHECK(weight_.size(0) == local_out_ && weight_.size(1) == local_in_ / 2, "loaded weight is [", weight_.size(0),
              ", ", weight_.size(1), "], expected [", local_out_, ", ", local_in_ / 2, "]");
  TORCH_CHECK(weight_scale_.size(0) == local_out_ && weight_scale_.size(1) == local_in_ / 32,
              "loaded weight_scale is [", weight_scale_.size(0), ", ", weight_scale_.size(1), "], expected [", local_out_,
              ", ", local_in_ / 32, "]");
}

torch::Tensor Mxfp4LinearHipBase::gemm(const torch::Tensor& input, bool with_bias) const {
  return slm::mxfp4_linear(input, weight_, weight_scale_,
                           with_bias && has_bias_ ? std::optional<torch::Tensor>(bias_) : std::nullopt, silu_mul_);
}

// ---------------------------------------------------------------------------------------------
ColumnParallelMxfp4LinearHipImpl::ColumnParallelMxfp4LinearHipImpl(int64_t in_features, int64_t out_features, bool bias,
                                                                   bool gather_output,
                                                                   const ParallelArgs& parallel_args,
                                                                   const torch::TensorOptions& options)
    : Mxfp4LinearHipBase(bias, parallel_args, options), in_features_(in_features), gather_output_(gather_output) {
  const int64_t world = parallel_args.world_size();
  TORCH_CHECK(out_features % world == 0, "out_features ", out_features, " not divisible by world_size ", world);
  local_in_ = in_features;
  local_out_ = out_features / world;
  TORCH_CHECK(local_out_ % 32 == 0 && local_in_ % 32 == 0, "mxfp4 shapes: N per rank % 32, K % 32");
}

void ColumnParallelMxfp4LinearHipImpl::load_state_dict(const StateDict& sd) {
  load_pair(sd, in_features_, 0);
  if (has_bias_) load_one(sd, "bias", 0, bias_, bias_is_loaded_);
}

void ColumnParallelMxfp4LinearHipImpl::load_state_dict(const StateDict& sd, const std::vector<std::string>& prefixes) {
  // per prefix the weight shard and its scale rows arrive together; both are concatenated on dim 0 once all prefixes
  // are there (q | k | v, gate | up)
  if (weight_list_.size() < prefixes.size()) {
    weight_list_.resize(prefixes.size());
    scale_list_.resize(prefixes.size());
  }
  for (size_t i = 0; i < prefixes.size(); ++i) {
    const auto w = bytes_of(sd, prefixes[i] + "weight", in_features_ / 2);
    const auto s = bytes_of(sd, prefixes[i] + "weight_scale", in_features_ / 32);
    if (!w.defined()) {
      TORCH_CHECK(!s.defined(), sd.prefix() + prefixes[i], "weight_scale arrives without its weight");
      continue;
    }
    TORCH_CHECK(!weight_list_[i].defined() && !weight_is_loaded_, "weight ", sd.prefix() + prefixes[i] + "weight",
                " is loaded twice");
    TORCH_CHECK(s.defined(), sd.prefix() + prefixes[i], "weight arrives without its weight_scale");
    TORCH_CHECK(s.size(0) == w.size(0), sd.prefix() + prefixes[i], "weight_scale has ", s.size(0), " rows for ",
                w.size(0), " weight rows");
    weight_list_[i] = shard(w, 0, prefixes[i] + "weight");
    scale_list_[i] = shard(s, 0, prefixes[i] + "weight_scale");
  }
  if (!weight_is_loaded_ &&
      std::all_of(weight_list_.begin(), weight_list_.end(), [](const torch::Tensor& t) { return t.defined(); })) {
    weight_ = torch::cat(weight_list_, 0).contiguous();
    weight_scale_ = torch::cat(scale_list_, 0).contiguous();
    weight_list_.clear();
    scale_list_.clear();
    weight_is_loaded_ = scale_is_loaded_ = true;
  }
  if (has_bias_) load_fused(sd, prefixes, "bias", bias_list_, bias_, bias_is_loaded_);
}

torch::Tensor ColumnParallelMxfp4LinearHipImpl::forward(torch::Tensor input) {
  verify_loaded_weights();
  auto out = gemm(input, /*with_bias=*/true);
  auto* pg = parallel_args_.process_group();
  if (parallel_args_.world_size() > 1 && gather_output_ && pg != nullptr) {
    std::vector<torch::Tensor> parts;
    for (int r = 0; r < parallel_args_.world_size(); ++r) parts.push_back(torch::empty_like(out));
    pg->allgather(out.contiguous(), parts);
    out = torch::cat(parts, /*dim=*/-1).contiguous();
  }
  return out;
}

// ---------------------------------------------------------------------------------------------
RowParallelMxfp4LinearHipImpl::RowParallelMxfp4LinearHipImpl(int64_t in_features, int64_t out_features, bool bias,
                                                             bool input_is_parallelized,
                                                             const ParallelArgs& parallel_args,
                                                             const torch::TensorOptions& options)
    : Mxfp4LinearHipBase(bias, parallel_args, options), in_features_(in_features),
      input_is_parallelized_(input_is_parallelized) {
  const int64_t world = parallel_args.world_size();
  TORCH_CHECK(in_features % world == 0, "in_features ", in_features, " not divisible by world_size ", world);
  local_in_ = in_features / world;
  local_out_ = out_features;
  TORCH_CHECK(local_out_ % 32 == 0 && local_in_ % 32 == 0, "mxfp4 shapes: N % 32, K per rank % 32 (whole MX blocks)");
}

void RowParallelMxfp4LinearHipImpl::load_state_dict(const StateDict& sd) {
  load_pair(sd, in_features_, 1);
  if (has_bias_) load_one(sd, "bias", -1, bias_, bias_is_loaded_);  // added once, after the reduction
}

void RowParallelMxfp4LinearHipImpl::load_state_dict(const StateDict&, const std::vector<std::string>&) {
  TORCH_CHECK(false, "row-parallel linears are never fused (parallel_linear.h:28-33)");
}

torch::Tensor RowParallelMxfp4LinearHipImpl::forward(torch::Tensor input) {
  verify_loaded_weights();
  const int world = parallel_args_.world_size();
  if (!input_is_parallelized_ && world > 1) {
    TORCH_CHECK(input.size(-1) % world == 0);
    input = input.chunk(world, /*dim=*/-1)[parallel_args_.rank()].contiguous();
  }
  if (world == 1) return gemm(input, /*with_bias=*/true);
  auto out = gemm(input, /*with_bias=*/false);  // partial sums
  auto* pg = parallel_args_.process_group();
  // process_group == nullptr with world_size > 1: the caller owns the reduction and gets this rank's PARTIAL sums
  if (pg == nullptr) {
    TORCH_CHECK(!has_bias_, "partial sums requested from a row-parallel linear with a bias");
    return out;
  }
  pg->allreduce(out);
  if (has_bias_) out.add_(bias_);  // the bias AFTER the reduce
  return out;
}

// ---------------------------------------------------------------------------------------------
std::shared_ptr<ColumnParallelMxfp4LinearHipImpl> create_column_parallel_mxfp4_linear(
    int64_t in_features, int64_t out_features, bool bias, bool gather_output, const ParallelArgs& parallel_args,
    const torch::TensorOptions& options) {
  return std::make_shared<ColumnParallelMxfp4LinearHipImpl>(in_features, out_features, bias, gather_output,
                                                            parallel_args, options);
}

std::shared_ptr<RowParallelMxfp4LinearHipImpl> create_row_parallel_mxfp4_linear(
    int64_t in_features, int64_t out_features, bool bias, bool input_is_parallelized,
    const ParallelArgs& parallel_args, const torch::TensorOptions& options) {
  return std::make_shared<RowParallelMxfp4LinearHipImpl>(in_features, out_features, bias, input_is_parallelized,
                                                         parallel_args, options);
}

}  // namespace slm
