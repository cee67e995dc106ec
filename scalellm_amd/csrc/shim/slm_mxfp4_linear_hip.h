// slm_mxfp4_linear_hip.h -- the OCP MXFP4 weight-only linear layers on the HIP kernel: the layer surface of
// slm_linear_hip.h over slm::mxfp4_linear (slm_torch_shim.h; include/slm_hip.h section 20, W4A16).
//
// A checkpoint brings `weight` (uint8 [out, in / 2], two e2m1 codes per byte, the low nibble the lower k; or the same
// bytes as [out, in / 32, 16] or float4_e2m1fn_x2) and `weight_scale` (uint8 or float8_e8m0fnu [out, in / 32], one
// e8m0 byte per 32 k); both are kept as bytes and never converted.  Sharding: column -- weight and scale on dim 0,
// fused prefixes concatenated on dim 0; row -- weight AND scale on dim 1 (the K shard is a multiple of 32), the bias
// added after the reduction.  A weight of another dtype is an error, never a silent quantisation.  Bit-identical to
// layers.ColumnParallelMxfp4Linear / RowParallelMxfp4Linear.
#pragma once
#include "slm_linear_hip.h"

namespace slm {

class Mxfp4LinearHipBase : public LinearHipBase {
 public:
  void verify_loaded_weights(const std::string& prefix = "") const override;
  torch::Tensor weight_scale() const { return weight_scale_; }

 protected:
  using LinearHipBase::LinearHipBase;
  // a checkpoint tensor as 2-D uint8 [rows, cols] (undefined when the dict does not hold it)
  static torch::Tensor bytes_of(const StateDict& sd, const std::string& name, int64_t cols);
  // this rank's chunk on `dim`, on the layer's device
  torch::Tensor shard(const torch::Tensor& t, int64_t dim, const std::string& what) const;
  void load_pair(const StateDict& sd, int64_t in_features, int64_t dim);
  torch::Tensor gemm(const torch::Tensor& input, bool with_bias) const;

  torch::Tensor weight_scale_;
  bool scale_is_loaded_ = false;
  std::vector<torch::Tensor> scale_list_;
};

class ColumnParallelMxfp4LinearHipImpl : public Mxfp4LinearHipBase {
 public:
  ColumnParallelMxfp4LinearHipImpl(int64_t in_features, int64_t out_features, bool bias, bool gather_output,
                                   const ParallelArgs& parallel_args, const torch::TensorOptions& options);
  torch::Tensor forward(torch::Tensor input) override;
  void load_state_dict(const StateDict& state_dict) override;
  void load_state_dict(const StateDict& state_dict, const std::vector<std::string>& prefixes) override;

 private:
  int64_t in_features_;
  bool gather_output_;
};

class RowParallelMxfp4LinearHipImpl : public Mxfp4LinearHipBase {
 public:
  RowParallelMxfp4LinearHipImpl(int64_t in_features, int64_t out_features, bool bias, bool input_is_parallelized,
                                const ParallelArgs& parallel_args, const torch::TensorOptions& options);
  torch::Tensor forward(torch::Tensor input) override;
  void load_state_dict(const StateDict& state_dict) override;
  void load_state_dict(const StateDict& state_dict, const std::vector<std::string>& prefixes) override;

 private:
  int64_t in_features_;
  bool input_is_parallelized_;
};

std::shared_ptr<ColumnParallelMxfp4LinearHipImpl> create_column_parallel_mxfp4_linear(
    int64_t in_features, int64_t out_features, bool bias, bool gather_output, const ParallelArgs& parallel_args,
    const torch::TensorOptions& options);
std::shared_ptr<RowParallelMxfp4LinearHipImpl> create_row_parallel_mxfp4_linear(
    int64_t in_features, int64_t out_features, bool bias, bool input_is_parallelized,
    const ParallelArgs& parallel_args, const torch::TensorOptions& options);

}  // namespace slm
