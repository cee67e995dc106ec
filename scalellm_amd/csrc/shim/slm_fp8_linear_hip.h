// slm_fp8_linear_hip.h -- the fp8 (e4m3) weight-only linear layers on the HIP kernel: the layer surface of
// slm_linear_hip.h over slm::fp8_linear (slm_torch_shim.h; include/slm_hip.h section 15, W8A16).
//
// A checkpoint brings `weight` (float8_e4m3fn [out, in], kept as bytes, never converted) and `weight_scale`
// (0-d, [1], [out] or [out, 1], any float dtype; kept as fp32 [out_per_rank], a per-tensor scale expanded -- in a
// fused load per shard); an `input_scale` is not read.  Sharding is the dense layers': column -- weight and scale
// on dim 0; row -- weight on dim 1, the scale whole, and with world_size > 1 the GEMM applies the scale, then the
// all-reduce, then the bias.  A weight of another dtype is an error, never a silent quantisation.  Bit-identical to
// layers.ColumnParallelFp8Linear / RowParallelFp8Linear.
#pragma once
#include "slm_linear_hip.h"

namespace slm {

class Fp8LinearHipBase : public LinearHipBase {
 public:
  void verify_loaded_weights(const std::string& prefix = "") const override;
  torch::Tensor weight_scale() const { return weight_scale_; }

 protected:
  using LinearHipBase::LinearHipBase;
  // this rank's shard of `weight` (dim < 0: whole), still float8_e4m3fn
  torch::Tensor fp8_shard(const StateDict& sd, const std::string& name, int64_t dim) const;
  // `weight_scale` as fp32 [rows]
  static torch::Tensor channel_scale(const torch::Tensor& t, int64_t rows, const std::string& what);
  void load_weight(const StateDict& sd, int64_t dim);
  void load_scale(const StateDict& sd, int64_t full_rows, bool shard);
  torch::Tensor gemm(const torch::Tensor& input, bool with_bias) const;

  torch::Tensor weight_scale_;
  bool scale_is_loaded_ = false;
  std::vector<torch::Tensor> scale_list_;
};

class ColumnParallelFp8LinearHipImpl : public Fp8LinearHipBase {
 public:
  ColumnParallelFp8LinearHipImpl(int64_t in_features, int64_t out_features, bool bias, bool gather_output,
                                 const ParallelArgs& parallel_args, const torch::TensorOptions& options);
  torch::Tensor forward(torch::Tensor input) override;
  void load_state_dict(const StateDict& state_dict) override;
  void load_state_dict(const StateDict& state_dict, const std::vector<std::string>& prefixes) override;

 private:
  int64_t out_features_;
  bool gather_output_;
};

class RowParallelFp8LinearHipImpl : public Fp8LinearHipBase {
 public:
  RowParallelFp8LinearHipImpl(int64_t in_features, int64_t out_features, bool bias, bool input_is_parallelized,
                              const ParallelArgs& parallel_args, const torch::TensorOptions& options);
  torch::Tensor forward(torch::Tensor input) override;
  void load_state_dict(const StateDict& state_dict) override;
  void load_state_dict(const StateDict& state_dict, const std::vector<std::string>& prefixes) override;

 private:
  bool input_is_parallelized_;
};

std::shared_ptr<ColumnParallelFp8LinearHipImpl> create_column_parallel_fp8_linear(
    int64_t in_features, int64_t out_features, bool bias, bool gather_output, const ParallelArgs& parallel_args,
    const torch::TensorOptions& options);
std::shared_ptr<RowParallelFp8LinearHipImpl> create_row_parallel_fp8_linear(
    int64_t in_features, int64_t out_features, bool bias, bool input_is_parallelized,
    const ParallelArgs& parallel_args, const torch::TensorOptions& options);

}  // namespace slm
