// slm_fp8_linear_hip.cpp -- see slm_fp8_linear_hip.h.  Host code only.
#include "slm_fp8_linear_hip.h"

#include <algorithm>

namespace slm {

torch::Tensor Fp8LinearHipBase::fp8_shard(const StateDict& sd, const std::string& name, int64_t dim) const {
  const auto t = dim < 0 ? sd.get_tensor(name)
                         : sd.get_sharded_tensor(name, dim, parallel_args_.rank(), parallel_args_.world_size());
  if (!t.defined()) return t;
  TORCH_CHECK(t.scalar_type() == torch::kFloat8_e4m3fn, "fp8 linear: ", sd.prefix() + name,
              " must be float8_e4m3fn, not ", t.scalar_type(), " (nothing is quantised on load)");
  return t.to(options_.device());
}

torch::Tensor Fp8LinearHipBase::channel_scale(const torch::Tensor& t, int64_t rows, const std::string& what) {
  TORCH_CHECK(t.is_floating_point(), what, " must be a float tensor, not ", t.scalar_type());
  auto flat = t.reshape({-1}).to(torch::kFloat);
  if (flat.numel() == 1) return flat.expand({rows});
  TORCH_CHECK(flat.numel() == rows && t.dim() <= 2 && (t.dim() < 2 || t.size(1) == 1), what, " size mismatch: ",
              t.sizes(), " for ", rows, " output channels");
  return flat;
}

void Fp8LinearHipBase::load_weight(const StateDict& sd, int64_t dim) {
  const auto t = fp8_shard(sd, "weight", dim);
  if (!t.defined()) return;
  TORCH_CHECK(!weight_is_loaded_, "weight ", sd.prefix() + "weight", " is loaded twice");
  weight_ = t.contiguous();
  weight_is_loaded_ = true;
}

void Fp8LinearHipBase::load_scale(const StateDict& sd, int64_t full_rows, bool shard) {
  const auto t = sd.get_tensor("weight_scale");
  if (!t.defined()) return;
  TORCH_CHECK(!scale_is_loaded_, "weight ", sd.prefix() + "weight_scale", " is loaded twice");
  auto full = channel_scale(t, full_rows, sd.prefix() + "weight_scale");
  const int world = parallel_args_.world_size();
  if (shard && world > 1) full = full.chunk(world, 0)[parallel_args_.rank()];
  weight_scale_ = full.to(options_.device()).contiguous();
  scale_is_loaded_ = true;
}

void Fp8LinearHipBase::verify_loaded_weights(const std::string& prefix) const {
  LinearHipBase::verify_loaded_weights(prefix);
  TORCH_CHECK(scale_is_loaded_, "weight_scale is not loaded for ", prefix + "weight_scale");
  TORCH_CHECK(weight_scale_.numel() == local_out_, "loaded weight_scale has ", weight_scale_.numel(),
              " entries, expected ", local_out_);
}

torch::Tensor Fp8LinearHipBase::gemm(const torch::Tensor& input, bool with_bias) const {
  return slm::fp8_linear(input, weight_, weight_scale_,
                         with_bias && has_bias_ ? std::optional<torch::Tensor>(bias_) : std::nullopt, silu_mul_);
}

// ---------------------------------------------------------------------------------------------
ColumnParallelFp8LinearHipImpl::ColumnParallelFp8LinearHipImpl(int64_t in_features, int64_t out_features, bool bias,
                                                               bool gather_output, const ParallelArgs& parallel_args,
                                                               const torch::TensorOptions& options)
    : Fp8LinearHipBase(bias, parallel_args, options), out_features_(out_features), gather_output_(gather_output) {
  const int64_t world = parallel_args.world_size();
  TORCH_CHECK(out_features % world == 0, "out_features ", out_features, " not divisible by world_size ", world);
  local_in_ = in_features;
  local_out_ = out_features / world;
  TORCH_CHECK(local_out_ % 32 == 0 && local_in_ % 32 == 0, "fp8 shapes: N per rank % 32, K % 32");
}

void ColumnParallelFp8LinearHipImpl::load_state_dict(const StateDict& sd) {
  load_weight(sd, 0);
  load_scale(sd, out_features_, /*shard=*/true);
  if (has_bias_) load_one(sd, "bias", 0, bias_, bias_is_loaded_);
}

void ColumnParallelFp8LinearHipImpl::load_state_dict(const StateDict& sd, const std::vector<std::string>& prefixes) {
  // per prefix the weight shard and its scale over the shard's rows arrive together; concatenated on dim 0 once all
  // prefixes are there (q | k | v, gate | up), every shard under its own scale
  if (weight_list_.size() < prefixes.size()) {
    weight_list_.resize(prefixes.size());
    scale_list_.resize(prefixes.size());
  }
  const int world = parallel_args_.world_size(), rank = parallel_args_.rank();
  for (size_t i = 0; i < prefixes.size(); ++i) {
    const auto full = sd.get_tensor(prefixes[i] + "weight");
    const auto sc = sd.get_tensor(prefixes[i] + "weight_scale");
    if (!full.defined()) {
      TORCH_CHECK(!sc.defined(), sd.prefix() + prefixes[i], "weight_scale arrives without its weight");
      continue;
    }
    TORCH_CHECK(!weight_list_[i].defined() && !weight_is_loaded_, "weight ", sd.prefix() + prefixes[i] + "weight",
                " is loaded twice");
    TORCH_CHECK(sc.defined(), sd.prefix() + prefixes[i], "weight arrives without its weight_scale");
    auto s = channel_scale(sc, full.size(0), sd.prefix() + prefixes[i] + "weight_scale");
    if (world > 1) {
      TORCH_CHECK(full.size(0) % world == 0, "can't divide ", prefixes[i], "weight evenly on dim 0");
      s = s.chunk(world, 0)[rank];
    }
    weight_list_[i] = fp8_shard(sd, prefixes[i] + "weight", 0).view(torch::kUInt8);
    scale_list_[i] = s.to(options_.device());
  }
  if (!weight_is_loaded_ &&
      std::all_of(weight_list_.begin(), weight_list_.end(), [](const torch::Tensor& t) { return t.defined(); })) {
    weight_ = torch::cat(weight_list_, 0).contiguous().view(torch::kFloat8_e4m3fn);
    weight_scale_ = torch::cat(scale_list_, 0).contiguous();
    weight_list_.clear();
    scale_list_.clear();
    weight_is_loaded_ = scale_is_loaded_ = true;
  }
  if (has_bias_) load_fused(sd, prefixes, "bias", bias_list_, bias_, bias_is_loaded_);
}

torch::Tensor ColumnParallelFp8LinearHipImpl::forward(torch::Tensor input) {
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
RowParallelFp8LinearHipImpl::RowParallelFp8LinearHipImpl(int64_t in_features, int64_t out_features, bool bias,
                                                         bool input_is_parallelized, const ParallelArgs& parallel_args,
                                                         const torch::TensorOptions& options)
    : Fp8LinearHipBase(bias, parallel_args, options), input_is_parallelized_(input_is_parallelized) {
  const int64_t world = parallel_args.world_size();
  TORCH_CHECK(in_features % world == 0, "in_features ", in_features, " not divisible by world_size ", world);
  local_in_ = in_features / world;
  local_out_ = out_features;
  TORCH_CHECK(local_out_ % 32 == 0 && local_in_ % 32 == 0, "fp8 shapes: N % 32, K per rank % 32");
}

void RowParallelFp8LinearHipImpl::load_state_dict(const StateDict& sd) {
  load_weight(sd, 1);
  load_scale(sd, local_out_, /*shard=*/false);
  if (has_bias_) load_one(sd, "bias", -1, bias_, bias_is_loaded_);  // added once, after the reduction
}

void RowParallelFp8LinearHipImpl::load_state_dict(const StateDict&, const std::vector<std::string>&) {
  TORCH_CHECK(false, "row-parallel linears are never fused (parallel_linear.h:28-33)");
}

torch::Tensor RowParallelFp8LinearHipImpl::forward(torch::Tensor input) {
  verify_loaded_weights();
  const int world = parallel_args_.world_size();
  if (!input_is_parallelized_ && world > 1) {
    TORCH_CHECK(input.size(-1) % world == 0);
    input = input.chunk(world, /*dim=*/-1)[parallel_args_.rank()].contiguous();
  }
  if (world == 1) return gemm(input, /*with_bias=*/true);
  auto out = gemm(input, /*with_bias=*/false);  // scaled partial sums
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
std::shared_ptr<ColumnParallelFp8LinearHipImpl> create_column_parallel_fp8_linear(
    int64_t in_features, int64_t out_features, bool bias, bool gather_output, const ParallelArgs& parallel_args,
    const torch::TensorOptions& options) {
  return std::make_shared<ColumnParallelFp8LinearHipImpl>(in_features, out_features, bias, gather_output, parallel_args,
                                                          options);
}

std::shared_ptr<RowParallelFp8LinearHipImpl> create_row_parallel_fp8_linear(
    int64_t in_features, int64_t out_features, bool bias, bool input_is_parallelized,
    const ParallelArgs& parallel_args, const torch::TensorOptions& options) {
  return std::make_shared<RowParallelFp8LinearHipImpl>(in_features, out_features, bias, input_is_parallelized,
                                                       parallel_args, options);
}

}  // namespace slm
