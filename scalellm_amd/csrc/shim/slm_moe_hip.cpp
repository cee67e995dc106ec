// slm_moe_hip.cpp -- see slm_moe_hip.h.  Host code only: tensors are unpacked into the C ABI's arguments and
// handed to the slm_moe_* entry points on torch's current HIP stream.
#include "slm_moe_hip.h"

#include <algorithm>

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include "slm_hip.h"

namespace {

void check(int rc, const char* what) {
  TORCH_CHECK(rc == SLM_OK, what, " failed: ", slm_status_string(rc), " (", rc, ")",
              rc == SLM_ERR_LAUNCH ? slm_last_hip_error() : "");
}

void* stream_of(const torch::Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

void check_i32(const torch::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt && t.is_contiguous(), "slm moe: ", what,
              " must be a contiguous int32 GPU tensor");
}

void check_route(const torch::Tensor& logits, const torch::Tensor& w, const torch::Tensor& idx) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.scalar_type() == torch::kFloat && logits.is_contiguous(),
              "slm moe: gating_logits must be a contiguous fp32 GPU [n_tokens, n_experts] tensor");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kFloat && w.is_contiguous() && w.dim() == 2 &&
                  w.size(0) == logits.size(0),
              "slm moe: topk_weights must be contiguous fp32 [n_tokens, topk]");
  check_i32(idx, "topk_indices");
  TORCH_CHECK(idx.sizes() == w.sizes(), "slm moe: topk_indices must have the shape of topk_weights");
}

int dtype_code(const torch::Tensor& t) {
  if (t.scalar_type() == torch::kBFloat16) return SLM_BF16;
  if (t.scalar_type() == torch::kHalf) return SLM_F16;
  TORCH_CHECK(false, "slm moe: fp16 / bf16 activations only, got ", t.scalar_type());
  return -1;
}

}  // namespace

namespace slm {

void moe_sum_add(const torch::Tensor& input, const torch::Tensor& addend, torch::Tensor& output) {
  TORCH_CHECK(input.is_cuda() && addend.is_cuda() && output.is_cuda() && input.dim() == 3 && input.is_contiguous() &&
                  addend.is_contiguous() && output.is_contiguous() && input.scalar_type() == output.scalar_type() &&
                  addend.scalar_type() == output.scalar_type() && output.dim() == 2 && addend.dim() == 2 &&
                  output.size(0) == input.size(0) && output.size(1) == input.size(2) &&
                  addend.size(0) == output.size(0) && addend.size(1) == output.size(1),
              "slm moe: moe_sum_add takes contiguous [n_tokens, topk, dim] + [n_tokens, dim] -> [n_tokens, dim] of one "
              "dtype");
  check(slm_moe_sum_add(output.data_ptr(), input.data_ptr(), addend.data_ptr(), input.size(0),
                        static_cast<int32_t>(input.size(1)), input.size(2), dtype_code(input), stream_of(input)),
        "slm_moe_sum_add");
}

void moe_topk_softmax(const torch::Tensor& gating_logits, torch::Tensor& topk_weights, torch::Tensor& topk_indices,
                      bool renormalize) {
  check_route(gating_logits, topk_weights, topk_indices);
  check(slm_moe_topk_softmax(gating_logits.const_data_ptr<float>(), topk_weights.data_ptr<float>(),
                             topk_indices.data_ptr<int32_t>(), gating_logits.size(0),
                             static_cast<int32_t>(gating_logits.size(1)), static_cast<int32_t>(topk_weights.size(-1)),
                             renormalize ? 1 : 0, stream_of(gating_logits)),
        "slm_moe_topk_softmax");
}

void moe_w4_grouped_gemm(const torch::Tensor& a, const torch::Tensor& wq, const torch::Tensor& sz, torch::Tensor& c,
                         const torch::Tensor& sorted_token_idxes, const torch::Tensor& expert_ids,
                         const torch::Tensor& n_padded_tokens, int64_t K, int64_t N, int64_t group_size,
                         int64_t a_div, int64_t format, const torch::Tensor& row_scale, bool silu_mul) {
  TORCH_CHECK(a.is_cuda() && c.is_cuda() && a.dim() == 2 && c.dim() == 2 && a.stride(1) == 1 && c.stride(1) == 1,
              "slm moe: A and C must be 2-D GPU tensors with contiguous rows");
  TORCH_CHECK(a.scalar_type() == c.scalar_type(), "slm moe: A and C must share a dtype");
  TORCH_CHECK(wq.is_cuda() && sz.is_cuda() && wq.dim() == 2 && sz.dim() == 2 && wq.size(0) == sz.size(0) &&
                  wq.stride(1) == 1 && sz.stride(1) == 1 && wq.element_size() == 4 && sz.element_size() == 4,
              "slm moe: wq / sz must be [n_experts, words] 32-bit GPU tensors");
  check_i32(sorted_token_idxes, "sorted_token_idxes");
  check_i32(expert_ids, "expert_ids");
  check_i32(n_padded_tokens, "n_padded_tokens");
  TORCH_CHECK(a.size(1) == K && c.size(1) == (silu_mul ? N / 2 : N) && a_div >= 1 && a.size(0) * a_div >= c.size(0),
              "slm moe: grouped GEMM shape mismatch");
  TORCH_CHECK(sorted_token_idxes.numel() >= expert_ids.numel() * 32,
              "slm moe: sorted_token_idxes is shorter than expert_ids.numel() blocks of 32");
  slm_moe_gemm_args g{};
  g.a = a.data_ptr();
  g.wq = wq.data_ptr();
  g.sz = sz.data_ptr();
  g.c = c.data_ptr();
  if (row_scale.defined()) {
    TORCH_CHECK(row_scale.is_cuda() && row_scale.scalar_type() == torch::kFloat && row_scale.is_contiguous() &&
                    row_scale.numel() == c.size(0),
                "slm moe: row_scale must be contiguous fp32 with one entry per row of C");
    g.row_scale = row_scale.const_data_ptr<float>();
  }
  g.sorted_token_idxes = sorted_token_idxes.const_data_ptr<int32_t>();
  g.expert_ids = expert_ids.const_data_ptr<int32_t>();
  g.n_padded_tokens = n_padded_tokens.const_data_ptr<int32_t>();
  g.wq_expert_stride = wq.stride(0) * 4;
  g.sz_expert_stride = sz.stride(0) * 4;
  g.n_flat = c.size(0);
  g.K = K;
  g.N = N;
  g.lda = a.stride(0);
  g.ldc = c.stride(0);
  g.group_size = group_size;
  g.a_div = static_cast<int32_t>(a_div);
  g.n_experts = static_cast<int32_t>(wq.size(0));
  g.max_blocks = static_cast<int32_t>(expert_ids.numel());
  g.dtype = dtype_code(a);
  g.format = static_cast<int32_t>(format);
  g.flags = silu_mul ? SLM_W4_SILU_MUL : 0;
  check(slm_moe_w4a16_gemm(&g, stream_of(a)), "slm_moe_w4a16_gemm");
}

void moe_grouped_gemm(const torch::Tensor& a, const torch::Tensor& w, torch::Tensor& c,
                      const torch::Tensor& sorted_token_idxes, const torch::Tensor& expert_ids,
                      const torch::Tensor& n_padded_tokens, int64_t a_div, const torch::Tensor& row_scale,
                      bool silu_mul) {
  TORCH_CHECK(a.is_cuda() && c.is_cuda() && a.dim() == 2 && c.dim() == 2 && a.stride(1) == 1 && c.stride(1) == 1,
              "slm moe: A and C must be 2-D GPU tensors with contiguous rows");
  TORCH_CHECK(w.is_cuda() && w.dim() == 3 && w.stride(2) == 1,
              "slm moe: expert weights must be a GPU tensor [n_experts, N, K] with k contiguous");
  TORCH_CHECK(a.scalar_type() == c.scalar_type() && a.scalar_type() == w.scalar_type(),
              "slm moe: A, W and C must share a dtype");
  check_i32(sorted_token_idxes, "sorted_token_idxes");
  check_i32(expert_ids, "expert_ids");
  check_i32(n_padded_tokens, "n_padded_tokens");
  const int64_t N = w.size(1), K = w.size(2);
  TORCH_CHECK(a.size(1) == K && c.size(1) == (silu_mul ? N / 2 : N) && a_div >= 1 && a.size(0) * a_div >= c.size(0),
              "slm moe: grouped GEMM shape mismatch");
  TORCH_CHECK(sorted_token_idxes.numel() >= expert_ids.numel() * 32,
              "slm moe: sorted_token_idxes is shorter than expert_ids.numel() blocks of 32");
  slm_moe_gemm_dense_args g{};
  g.a = a.data_ptr();
  g.w = w.data_ptr();
  g.c = c.data_ptr();
  if (row_scale.defined()) {
    TORCH_CHECK(row_scale.is_cuda() && row_scale.scalar_type() == torch::kFloat && row_scale.is_contiguous() &&
                    row_scale.numel() == c.size(0),
                "slm moe: row_scale must be contiguous fp32 with one entry per row of C");
    g.row_scale = row_scale.const_data_ptr<float>();
  }
  g.sorted_token_idxes = sorted_token_idxes.const_data_ptr<int32_t>();
  g.expert_ids = expert_ids.const_data_ptr<int32_t>();
  g.n_padded_tokens = n_padded_tokens.const_data_ptr<int32_t>();
  // a single expert's stride(0) is not meaningful: any value covering the expert will do
  g.w_expert_stride = w.size(0) > 1 ? w.stride(0) : std::max(w.stride(0), (N - 1) * w.stride(1) + K);
  g.n_flat = c.size(0);
  g.K = K;
  g.N = N;
  g.lda = a.stride(0);
  g.ldw = w.stride(1);
  g.ldc = c.stride(0);
  g.a_div = static_cast<int32_t>(a_div);
  g.n_experts = static_cast<int32_t>(w.size(0));
  g.max_blocks = static_cast<int32_t>(expert_ids.numel());
  g.dtype = dtype_code(a);
  g.flags = silu_mul ? SLM_MOE_SILU_MUL : 0;
  check(slm_moe_gemm(&g, stream_of(a)), "slm_moe_gemm");
}

void moe_fp8_grouped_gemm(const torch::Tensor& a, const torch::Tensor& w8, const torch::Tensor& w_scale,
                          torch::Tensor& c, const torch::Tensor& sorted_token_idxes, const torch::Tensor& expert_ids,
                          const torch::Tensor& n_padded_tokens, int64_t a_div, const torch::Tensor& row_scale,
                          bool silu_mul) {
  TORCH_CHECK(a.is_cuda() && c.is_cuda() && a.dim() == 2 && c.dim() == 2 && a.stride(1) == 1 && c.stride(1) == 1,
              "slm moe: A and C must be 2-D GPU tensors with contiguous rows");
  TORCH_CHECK(w8.is_cuda() && w8.dim() == 3 && w8.stride(2) == 1,
              "slm moe: expert weights must be a GPU tensor [n_experts, N, K] with k contiguous");
  TORCH_CHECK(w8.scalar_type() == torch::kFloat8_e4m3fn || w8.scalar_type() == torch::kByte,
              "slm moe: fp8 expert weights must be float8_e4m3fn (or their bytes as uint8), got ", w8.scalar_type());
  TORCH_CHECK(a.scalar_type() == c.scalar_type(), "slm moe: A and C must share a dtype");
  check_i32(sorted_token_idxes, "sorted_token_idxes");
  check_i32(expert_ids, "expert_ids");
  check_i32(n_padded_tokens, "n_padded_tokens");
  const int64_t E = w8.size(0), N = w8.size(1), K = w8.size(2);
  TORCH_CHECK(a.size(1) == K && c.size(1) == (silu_mul ? N / 2 : N) && a_div >= 1 && a.size(0) * a_div >= c.size(0),
              "slm moe: grouped GEMM shape mismatch");
  TORCH_CHECK(sorted_token_idxes.numel() >= expert_ids.numel() * 32,
              "slm moe: sorted_token_idxes is shorter than expert_ids.numel() blocks of 32");
  slm_moe_fp8_gemm_args g{};
  g.a = a.data_ptr();
  g.w = w8.data_ptr();
  g.c = c.data_ptr();
  if (w_scale.defined()) {
    TORCH_CHECK(w_scale.is_cuda() && w_scale.scalar_type() == torch::kFloat && w_scale.dim() == 2 &&
                    w_scale.size(0) == E && w_scale.size(1) == N && w_scale.stride(1) == 1,
                "slm moe: w_scale must be fp32 [n_experts, N] with contiguous rows");
    g.w_scale = w_scale.const_data_ptr<float>();
    g.w_scale_expert_stride = E > 1 ? w_scale.stride(0) : std::max(w_scale.stride(0), N);
  }
  if (row_scale.defined()) {
    TORCH_CHECK(row_scale.is_cuda() && row_scale.scalar_type() == torch::kFloat && row_scale.is_contiguous() &&
                    row_scale.numel() == c.size(0),
                "slm moe: row_scale must be contiguous fp32 with one entry per row of C");
    g.row_scale = row_scale.const_data_ptr<float>();
  }
  g.sorted_token_idxes = sorted_token_idxes.const_data_ptr<int32_t>();
  g.expert_ids = expert_ids.const_data_ptr<int32_t>();
  g.n_padded_tokens = n_padded_tokens.const_data_ptr<int32_t>();
  // a single expert's stride(0) is not meaningful: any multiple of 16 covering the expert will do
  g.w_expert_stride = E > 1 ? w8.stride(0) : std::max(w8.stride(0), N * w8.stride(1));
  g.n_flat = c.size(0);
  g.K = K;
  g.N = N;
  g.lda = a.stride(0);
  g.ldw = w8.stride(1);
  g.ldc = c.stride(0);
  g.a_div = static_cast<int32_t>(a_div);
  g.n_experts = static_cast<int32_t>(E);
  g.max_blocks = static_cast<int32_t>(expert_ids.numel());
  g.dtype = dtype_code(a);
  g.flags = silu_mul ? SLM_MOE_SILU_MUL : 0;
  check(slm_moe_fp8_gemm(&g, stream_of(a)), "slm_moe_fp8_gemm");
}

void moe_mxfp4_grouped_gemm(const torch::Tensor& a, const torch::Tensor& w, const torch::Tensor& w_scale,
                            torch::Tensor& c, const torch::Tensor& sorted_token_idxes,
                            const torch::Tensor& expert_ids, const torch::Tensor& n_padded_tokens, int64_t a_div,
                            const torch::Tensor& row_scale, bool silu_mul) {
  TORCH_CHECK(a.is_cuda() && c.is_cuda() && a.dim() == 2 && c.dim() == 2 && a.stride(1) == 1 && c.stride(1) == 1,
              "slm moe: A and C must be 2-D GPU tensors with contiguous rows");
  TORCH_CHECK(w.is_cuda() && w.dim() == 3 && w.stride(2) == 1 && w.scalar_type() == torch::kByte,
              "slm moe: mxfp4 expert weights must be a uint8 GPU tensor [n_experts, N, K/2] with k contiguous");
  TORCH_CHECK(a.scalar_type() == c.scalar_type(), "slm moe: A and C must share a dtype");
  check_i32(sorted_token_idxes, "sorted_token_idxes");
  check_i32(expert_ids, "expert_ids");
  check_i32(n_padded_tokens, "n_padded_tokens");
  const int64_t E = w.size(0), N = w.size(1), K = 2 * w.size(2);
  TORCH_CHECK(w_scale.defined() && w_scale.is_cuda() && w_scale.scalar_type() == torch::kByte && w_scale.dim() == 3 &&
                  K % 32 == 0 && w_scale.size(0) == E && w_scale.size(1) == N && w_scale.size(2) == K / 32 &&
                  w_scale.stride(2) == 1,
              "slm moe: mxfp4 w_scale must be uint8 [n_experts, N, K/32] e8m0 bytes with k contiguous");
  TORCH_CHECK(a.size(1) == K && c.size(1) == (silu_mul ? N / 2 : N) && a_div >= 1 && a.size(0) * a_div >= c.size(0),
              "slm moe: grouped GEMM shape mismatch");
  TORCH_CHECK(sorted_token_idxes.numel() >= expert_ids.numel() * 32,
              "slm moe: sorted_token_idxes is shorter than expert_ids.numel() blocks of 32");
  slm_moe_mxfp4_gemm_args g{};
  g.a = a.data_ptr();
  g.w = w.data_ptr();
  g.w_scale = w_scale.const_data_ptr<uint8_t>();
  g.c = c.data_ptr();
  if (row_scale.defined()) {
    TORCH_CHECK(row_scale.is_cuda() && row_scale.scalar_type() == torch::kFloat && row_scale.is_contiguous() &&
                    row_scale.numel() == c.size(0),
                "slm moe: row_scale must be contiguous fp32 with one entry per row of C");
    g.row_scale = row_scale.const_data_ptr<float>();
  }
  g.sorted_token_idxes = sorted_token_idxes.const_data_ptr<int32_t>();
  g.expert_ids = expert_ids.const_data_ptr<int32_t>();
  g.n_padded_tokens = n_padded_tokens.const_data_ptr<int32_t>();
  // a single expert's stride(0) is not meaningful: what covers the expert will do (the weights: a multiple of 16)
  g.w_expert_stride = E > 1 ? w.stride(0) : std::max(w.stride(0), N * w.stride(1));
  g.w_scale_expert_stride = E > 1 ? w_scale.stride(0) : std::max(w_scale.stride(0), N * w_scale.stride(1));
  g.n_flat = c.size(0);
  g.K = K;
  g.N = N;
  g.lda = a.stride(0);
  g.ldw = w.stride(1);
  g.ldc = c.stride(0);
  g.lds = w_scale.stride(1);
  g.a_div = static_cast<int32_t>(a_div);
  g.n_experts = static_cast<int32_t>(E);
  g.max_blocks = static_cast<int32_t>(expert_ids.numel());
  g.dtype = dtype_code(a);
  g.flags = silu_mul ? SLM_MOE_SILU_MUL : 0;
  check(slm_moe_mxfp4_gemm(&g, stream_of(a)), "slm_moe_mxfp4_gemm");
}

void moe_router(const torch::Tensor& x, const torch::Tensor& gate_weight, torch::Tensor& topk_weights,
                torch::Tensor& topk_indices, const std::string& scoring, bool renormalize,
                const torch::Tensor& correction_bias, int64_t n_expert_groups, int64_t topk_group,
                double scaling_factor, const torch::Tensor& logits_out) {
  TORCH_CHECK(scoring == "softmax" || scoring == "grouped_sigmoid", "slm moe: unknown scoring ", scoring);
  TORCH_CHECK(x.is_cuda() && gate_weight.is_cuda() && x.dim() == 2 && gate_weight.dim() == 2 && x.stride(1) == 1 &&
                  gate_weight.stride(1) == 1 && x.size(1) == gate_weight.size(1),
              "slm moe: router takes GPU x [n_tokens, hidden] and gate_weight [n_experts, hidden], contiguous rows");
  TORCH_CHECK(x.scalar_type() == gate_weight.scalar_type(), "slm moe: x and gate_weight must share a dtype");
  const int64_t T = x.size(0), H = x.size(1), E = gate_weight.size(0);
  TORCH_CHECK(topk_weights.is_cuda() && topk_weights.scalar_type() == torch::kFloat && topk_weights.is_contiguous() &&
                  topk_weights.dim() == 2 && topk_weights.size(0) == T,
              "slm moe: topk_weights must be contiguous fp32 [n_tokens, topk]");
  check_i32(topk_indices, "topk_indices");
  TORCH_CHECK(topk_indices.sizes() == topk_weights.sizes(),
              "slm moe: topk_indices must have the shape of topk_weights");
  slm_moe_router_args a{};
  a.x = x.data_ptr();
  a.gate_w = gate_weight.data_ptr();
  if (correction_bias.defined()) {
    TORCH_CHECK(correction_bias.is_cuda() && correction_bias.scalar_type() == torch::kFloat &&
                    correction_bias.is_contiguous() && correction_bias.numel() == E,
                "slm moe: correction_bias must be contiguous fp32 [n_experts]");
    a.correction_bias = correction_bias.const_data_ptr<float>();
  }
  a.weights = topk_weights.data_ptr<float>();
  a.indices = topk_indices.data_ptr<int32_t>();
  if (logits_out.defined()) {
    TORCH_CHECK(logits_out.is_cuda() && logits_out.scalar_type() == torch::kFloat && logits_out.is_contiguous() &&
                    logits_out.dim() == 2 && logits_out.size(0) == T && logits_out.size(1) == E,
                "slm moe: logits_out must be contiguous fp32 [n_tokens, n_experts]");
    a.logits_out = logits_out.data_ptr<float>();
  }
  a.n_tokens = T;
  a.hidden = H;
  a.ldx = T > 1 ? x.stride(0) : std::max(x.stride(0), H);
  a.ldw = E > 1 ? gate_weight.stride(0) : std::max(gate_weight.stride(0), H);
  a.n_experts = static_cast<int32_t>(E);
  a.topk = static_cast<int32_t>(topk_weights.size(1));
  a.dtype = dtype_code(x);
  a.scoring = scoring == "softmax" ? 0 : 1;
  a.renormalize = renormalize ? 1 : 0;
  a.n_expert_groups = static_cast<int32_t>(n_expert_groups);
  a.topk_group = static_cast<int32_t>(topk_group);
  a.scaling_factor = static_cast<float>(scaling_factor);
  size_t need = 0;
  check(slm_moe_router_workspace_bytes(T, a.n_experts, H, a.dtype, &need), "slm_moe_router_workspace_bytes");
  TORCH_CHECK(need == 0, "slm moe: the router plans a workspace this shim does not hold");
  check(slm_moe_router(&a, stream_of(x)), "slm_moe_router");
}

}  // namespace slm

namespace llm::kernel {

void topk_softmax(const torch::Tensor& gating_logits, torch::Tensor& topk_weights, torch::Tensor& topk_indices) {
  slm::moe_topk_softmax(gating_logits, topk_weights, topk_indices, /*renormalize=*/false);
}

void grouped_topk_sigmoid(const torch::Tensor& gating_logits, const torch::Tensor& correction_bias,
                          const int n_expert_groups, const int topk_group, const int topk, float scaling_factor,
                          torch::Tensor& topk_weights, torch::Tensor& topk_indices) {
  check_route(gating_logits, topk_weights, topk_indices);
  TORCH_CHECK(topk_weights.size(-1) == topk, "slm moe: topk_weights must be [n_tokens, topk]");
  TORCH_CHECK(correction_bias.is_cuda() && correction_bias.scalar_type() == torch::kFloat &&
                  correction_bias.is_contiguous() && correction_bias.numel() == gating_logits.size(1),
              "slm moe: correction_bias must be contiguous fp32 [n_experts]");
  check(slm_moe_grouped_topk_sigmoid(gating_logits.const_data_ptr<float>(), correction_bias.const_data_ptr<float>(),
                                     topk_weights.data_ptr<float>(), topk_indices.data_ptr<int32_t>(),
                                     gating_logits.size(0), static_cast<int32_t>(gating_logits.size(1)),
                                     n_expert_groups, topk_group, topk, scaling_factor, stream_of(gating_logits)),
        "slm_moe_grouped_topk_sigmoid");
}

namespace moe {

void permute_align_block(torch::Tensor topk_ids, int64_t n_experts, int64_t block_size,
                         torch::Tensor sorted_token_idxes, torch::Tensor experts_ids, torch::Tensor n_padded_tokens,
                         torch::Tensor cu_sum) {
  check_i32(topk_ids, "topk_ids");
  check_i32(sorted_token_idxes, "sorted_token_idxes");
  check_i32(experts_ids, "experts_ids");
  check_i32(n_padded_tokens, "n_padded_tokens");
  slm_moe_align_args a{};
  a.topk_ids = topk_ids.const_data_ptr<int32_t>();
  a.sorted_token_idxes = sorted_token_idxes.data_ptr<int32_t>();
  a.expert_ids = experts_ids.data_ptr<int32_t>();
  a.n_padded_tokens = n_padded_tokens.data_ptr<int32_t>();
  if (cu_sum.defined() && cu_sum.numel() > 0) {
    check_i32(cu_sum, "cu_sum");
    TORCH_CHECK(cu_sum.numel() >= n_experts + 1, "slm moe: cu_sum needs n_experts + 1 entries");
    a.cu_sum = cu_sum.data_ptr<int32_t>();
  }
  a.n_flat = topk_ids.numel();
  a.sorted_capacity = sorted_token_idxes.numel();
  a.blocks_capacity = experts_ids.numel();
  a.n_experts = static_cast<int32_t>(n_experts);
  a.block_size = static_cast<int32_t>(block_size);
  check(slm_moe_align_block(&a, stream_of(topk_ids)), "slm_moe_align_block");
}

void sum_out(const torch::Tensor& input, torch::Tensor& output) {
  TORCH_CHECK(input.is_cuda() && output.is_cuda() && input.dim() == 3 && input.is_contiguous() &&
                  output.is_contiguous() && input.scalar_type() == output.scalar_type() && output.dim() == 2 &&
                  output.size(0) == input.size(0) && output.size(1) == input.size(2),
              "slm moe: sum_out takes contiguous [n_tokens, topk, dim] -> [n_tokens, dim] of one dtype");
  check(slm_moe_sum(output.data_ptr(), input.data_ptr(), input.size(0), static_cast<int32_t>(input.size(1)),
                    input.size(2), dtype_code(input), stream_of(input)),
        "slm_moe_sum");
}

}  // namespace moe
}  // namespace llm::kernel
