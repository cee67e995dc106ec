// slm_linear_hip.cpp -- see slm_linear_hip.h.  Host code only.
#include "slm_linear_hip.h"

#include <algorithm>

namespace slm {

LinearHipBase::LinearHipBase(bool bias, const ParallelArgs& parallel_args, const torch::TensorOptions& options)
    : parallel_args_(parallel_args), options_(options), has_bias_(bias) {
  TORCH_CHECK(parallel_args.world_size() >= 1 && parallel_args.rank() >= 0 &&
              parallel_args.rank() < parallel_args.world_size(), "bad ParallelArgs");
  const auto dt = c10::typeMetaToScalarType(options.dtype());
  TORCH_CHECK(dt == torch::kHalf || dt == torch::kBFloat16, "slm: only fp16 / bf16 linears are supported, got ", dt);
}

void LinearHipBase::load_one(const StateDict& sd, const std::string& name, int64_t dim, torch::Tensor& dst,
                             bool& loaded) {
  // WeightUtils::load_sharded_weight (weight_utils.h:60-66): absent tensors are skipped
  const auto t = dim < 0 ? sd.get_tensor(name)
                         : sd.get_sharded_tensor(name, dim, parallel_args_.rank(), parallel_args_.world_size());
  if (!t.defined()) return;
  TORCH_CHECK(!loaded, "weight ", sd.prefix() + name, " is loaded twice");
  dst = t.to(options_.device(), c10::typeMetaToScalarType(options_.dtype())).contiguous();
  loaded = true;
}

void LinearHipBase::load_fused(const StateDict& sd, const std::vector<std::string>& prefixes, const std::string& name,
                               std::vector<torch::Tensor>& parts, torch::Tensor& dst, bool& loaded) {
  // WeightUtils::load_fused_weight (weight_utils.h:48-58): one shard per prefix, kept until all prefixes
  // have arrived, then concatenated on dim 0 (q | k | v, gate | up)
  if (parts.size() < prefixes.size()) parts.resize(prefixes.size());
  for (size_t i = 0; i < prefixes.size(); ++i) {
    const auto t = sd.get_sharded_tensor(prefixes[i] + name, 0, parallel_args_.rank(), parallel_args_.world_size());
    if (!t.defined()) continue;
    TORCH_CHECK(!parts[i].defined() && !loaded, "weight ", sd.prefix() + prefixes[i] + name, " is loaded twice");
    parts[i] = t.to(options_.device(), c10::typeMetaToScalarType(options_.dtype()));
  }
  if (!loaded && std::all_of(parts.begin(), parts.end(), [](const torch::Tensor& t) { return t.defined(); })) {
    dst = torch::cat(parts, 0).contiguous();
    parts.clear();
    loaded = true;
  }
}

void LinearHipBase::verify_loaded_weights(const std::string& prefix) const {
  TORCH_CHECK(weight_is_loaded_, "weight is not loaded for ", prefix + "weight");
  TORCH_CHECK(!has_bias_ || bias_is_loaded_, "bias is not loaded for ", prefix + "bias");
  TORCH_CHECK(weight_.size(0) == local_out_ && weight_.size(1) == local_in_, "loaded weight is [", weight_.size(0),
              ", ", weight_.size(1), "], expected [", local_out_, ", ", local_in_, "]");
}

// ---------------------------------------------------------------------------------------------
// column parallel: Y = X W^T + b, W [out, in] sharded along dim 0 (parallel_linear.cpp:221-263)
// ---------------------------------------------------------------------------------------------
ColumnParallelLinearHipImpl::ColumnParallelLinearHipImpl(int64_t in_features, int64_t out_features, bool bias,
                                                         bool gather_output, const ParallelArgs& parallel_args,
                                                         const torch::TensorOptions& options, const std::string&)
    : LinearHipBase(bias, parallel_args, options), gather_output_(gather_output) {
  const int64_t world = parallel_args.world_size();
  TORCH_CHECK(out_features % world == 0, "out_features ", out_features, " not divisible by world_size ", world);
  local_in_ = in_features;
  local_out_ = out_features / world;
  TORCH_CHECK(local_out_ % 32 == 0 && local_in_ % 32 == 0, "dense shapes: N per rank % 32, K % 32");
}

void ColumnParallelLinearHipImpl::load_state_dict(const StateDict& sd) {
  load_one(sd, "weight", 0, weight_, weight_is_loaded_);
  if (has_bias_) load_one(sd, "bias", 0, bias_, bias_is_loaded_);
}

void ColumnParallelLinearHipImpl::load_state_dict(const StateDict& sd, const std::vector<std::string>& prefixes) {
  load_fused(sd, prefixes, "weight", weight_list_, weight_, weight_is_loaded_);
  if (has_bias_) load_fused(sd, prefixes, "bias", bias_list_, bias_, bias_is_loaded_);
}

torch::Tensor ColumnParallelLinearHipImpl::forward(torch::Tensor input) {
  verify_loaded_weights();
  auto out = slm::linear(input, weight_, has_bias_ ? std::optional<torch::Tensor>(bias_) : std::nullopt, silu_mul_);
  auto* pg = parallel_args_.process_group();
  if (parallel_args_.world_size() > 1 && gather_output_ && pg != nullptr) {
    // gather_from_model_parallel_region (model_parallel.cpp:13-31): all-gather, concat on the last dim
    std::vector<torch::Tensor> parts;
    for (int r = 0; r < parallel_args_.world_size(); ++r) parts.push_back(torch::empty_like(out));
    pg->allgather(out.contiguous(), parts);
    out = torch::cat(parts, /*dim=*/-1).contiguous();
  }
  return out;
}

// ---------------------------------------------------------------------------------------------
// row parallel: Y = sum_r X_r W_r^T + b, W [out, in] sharded along dim 1 (parallel_linear.cpp:266-308)
// ---------------------------------------------------------------------------------------------
RowParallelLinearHipImpl::RowParallelLinearHipImpl(int64_t in_features, int64_t out_features, bool bias,
                                                   bool input_is_parallelized, const ParallelArgs& parallel_args,
                                                   const torch::TensorOptions& options)
    : LinearHipBase(bias, parallel_args, options), input_is_parallelized_(input_is_parallelized) {
  const int64_t world = parallel_args.world_size();
  TORCH_CHECK(in_features % world == 0, "in_features ", in_features, " not divisible by world_size ", world);
  local_in_ = in_features / world;
  local_out_ = out_features;
  TORCH_CHECK(local_out_ % 32 == 0 && local_in_ % 32 == 0, "dense shapes: N % 32, K per rank % 32");
}

void RowParallelLinearHipImpl::load_state_dict(const StateDict& sd) {
  load_one(sd, "weight", 1, weight_, weight_is_loaded_);
  if (has_bias_) load_one(sd, "bias", -1, bias_, bias_is_loaded_);  // added once, after the reduction
}

void RowParallelLinearHipImpl::load_state_dict(const StateDict&, const std::vector<std::string>&) {
  TORCH_CHECK(false, "row-parallel linears are never fused (parallel_linear.h:28-33)");
}

torch::Tensor RowParallelLinearHipImpl::forward(torch::Tensor input) {
  verify_loaded_weights();
  const int world = parallel_args_.world_size();
  if (!input_is_parallelized_ && world > 1) {
    // scatter_to_model_parallel_region (model_parallel.cpp:46-65): local split of the last dim
    TORCH_CHECK(input.size(-1) % world == 0);
    input = input.chunk(world, /*dim=*/-1)[parallel_args_.rank()].contiguous();
  }
  auto* pg = parallel_args_.process_group();
  if (world > 1) {
    auto out = slm::linear(input, weight_, std::nullopt);
    // process_group == nullptr with world_size > 1: the caller owns the reduction and gets this rank's PARTIAL sums
    if (pg == nullptr) {
      TORCH_CHECK(!has_bias_, "partial sums requested from a row-parallel linear with a bias");
      return out;
    }
    pg->allreduce(out);              // reduce_from_model_parallel_region (model_parallel.cpp:33-44)
    if (has_bias_) out.add_(bias_);  // N.B. the bias AFTER the reduce (parallel_linear.cpp:303-306)
    return out;
  }
  return slm::linear(input, weight_, has_bias_ ? std::optional<torch::Tensor>(bias_) : std::nullopt);
}

// ---------------------------------------------------------------------------------------------
std::shared_ptr<ParallelLinearImpl> create_column_parallel_linear(
    int64_t in_features, int64_t out_features, bool bias, bool gather_output, const QuantArgs& quant_args,
    const ParallelArgs& parallel_args, const torch::TensorOptions& options, const std::string& prefix) {
  if (!quant_args.quant_method().empty())
    return create_column_parallel_qlinear(in_features, out_features, bias, gather_output, quant_args, parallel_args,
                                          options);
  return std::make_shared<ColumnParallelLinearHipImpl>(in_features, out_features, bias, gather_output, parallel_args,
                                                       options, prefix);
}

std::shared_ptr<ParallelLinearImpl> create_row_parallel_linear(
    int64_t in_features, int64_t out_features, bool bias, bool input_is_parallelized, const QuantArgs& quant_args,
    const ParallelArgs& parallel_args, const torch::TensorOptions& options) {
  if (!quant_args.quant_method().empty())
    return create_row_parallel_qlinear(in_features, out_features, bias, input_is_parallelized, quant_args,
                                       parallel_args, options);
  return std::make_shared<RowParallelLinearHipImpl>(in_features, out_features, bias, input_is_parallelized,
                                                    parallel_args, options);
}

}  // namespace slm
