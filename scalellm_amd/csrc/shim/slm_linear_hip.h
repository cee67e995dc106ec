// slm_linear_hip.h -- the UNQUANTISED linear layers of the reference on the HIP kernel:
//
//   {Column,Row}ParallelLinearImpl        src/layers/linear/parallel_linear.{h,cpp}:221-308
//   create_{column,row}_parallel_linear   src/layers/linear/parallel_linear.cpp:167-217
//
// ColumnParallelLinearHipImpl / RowParallelLinearHipImpl are what the factory returns for an empty
// quant_method in an MI355X build: the reference's constructor argument order, the same virtual
// interface (ParallelLinearImpl of slm_qlinear_hip.h, untouched), the same TP sharding (column:
// weight and bias on dim 0, fused prefixes concatenated on dim 0; row: weight on dim 1, bias whole and
// added AFTER the reduction).  weight_ is the checkpoint tensor [out_per_rank, in] of the layer's
// dtype: slm_linear (include/slm_hip.h section 13) streams it as it is, there is no repack.
#pragma once
#include "slm_qlinear_hip.h"

namespace slm {

class LinearHipBase : public ParallelLinearImpl {
 public:
  void verify_loaded_weights(const std::string& prefix = "") const override;
  // this rank's shard [out_per_rank, in_per_rank] (testing)
  torch::Tensor weight() const { return weight_; }
  // The merged gate|up projection of the MLP: forward returns silu(gate) * up from the GEMM epilogue
  void set_act_mul_silu() { silu_mul_ = true; }

 protected:
  LinearHipBase(bool bias, const ParallelArgs& parallel_args, const torch::TensorOptions& options);
  // one tensor of one layer; dim < 0 = replicated
  void load_one(const StateDict& sd, const std::string& name, int64_t dim, torch::Tensor& dst, bool& loaded);
  void load_fused(const StateDict& sd, const std::vector<std::string>& prefixes, const std::string& name,
                  std::vector<torch::Tensor>& parts, torch::Tensor& dst, bool& loaded);

  ParallelArgs parallel_args_;
  torch::TensorOptions options_;
  bool has_bias_ = false, silu_mul_ = false;
  torch::Tensor weight_, bias_;
  bool weight_is_loaded_ = false, bias_is_loaded_ = false;
  std::vector<torch::Tensor> weight_list_, bias_list_;
  int64_t local_in_ = 0, local_out_ = 0;
};

class ColumnParallelLinearHipImpl : public LinearHipBase {
 public:
  ColumnParallelLinearHipImpl(int64_t in_features, int64_t out_features, bool bias, bool gather_output,
                              const ParallelArgs& parallel_args, const torch::TensorOptions& options,
                              const std::string& prefix = "");
  torch::Tensor forward(torch::Tensor input) override;
  void load_state_dict(const StateDict& state_dict) override;
  void load_state_dict(const StateDict& state_dict, const std::vector<std::string>& prefixes) override;

 private:
  bool gather_output_;
};

class RowParallelLinearHipImpl : public LinearHipBase {
 public:
  RowParallelLinearHipImpl(int64_t in_features, int64_t out_features, bool bias, bool input_is_parallelized,
                           const ParallelArgs& parallel_args, const torch::TensorOptions& options);
  torch::Tensor forward(torch::Tensor input) override;
  void load_state_dict(const StateDict& state_dict) override;
  void load_state_dict(const StateDict& state_dict, const std::vector<std::string>& prefixes) override;

 private:
  bool input_is_parallelized_;
};

// parallel_linear.cpp:167-217: a quant method -> the int4 factories of slm_qlinear_hip.h (which refuse
// anything but gptq / awq / GEMM), none -> the dense HIP impls
std::shared_ptr<ParallelLinearImpl> create_column_parallel_linear(
    int64_t in_features, int64_t out_features, bool bias, bool gather_output, const QuantArgs& quant_args,
    const ParallelArgs& parallel_args, const torch::TensorOptions& options, const std::string& prefix = "");
std::shared_ptr<ParallelLinearImpl> create_row_parallel_linear(
    int64_t in_features, int64_t out_features, bool bias, bool input_is_parallelized, const QuantArgs& quant_args,
    const ParallelArgs& parallel_args, const torch::TensorOptions& options);

}  // namespace slm
