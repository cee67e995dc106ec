// moe.hip -- mixture-of-experts routing and bookkeeping (include/slm_hip.h section 10):
//   slm_moe_topk_softmax         <- llm::kernel::topk_softmax          (moe/topk_softmax_kernel.cu:272)
//   slm_moe_grouped_topk_sigmoid <- llm::kernel::grouped_topk_sigmoid  (moe/grouped_topk_sigmoid_kernel.cu:280)
//   slm_moe_align_block          <- llm::kernel::moe::permute_align_block (moe/align_block_kernel.cu:192)
//   slm_moe_sum                  <- llm::kernel::moe::sum_out             (moe/align_block_kernel.cu:242)
//   slm_moe_sum_add              the same with one more row per token (the shared experts' output) added last
// Small kernels: one launch each, no float atomics, fixed reduction orders (bit-identical repeats).
// The grouped GEMM that consumes the aligned blocks is w4_moe.hip.
#include "common.h"
#include "moe_route.h"

namespace slm {
namespace {

constexpr int kMaxAlignExperts = 1024;

// one wave per token; the per-token bodies are moe_route.h's (shared with moe_router.hip)
__global__ void __launch_bounds__(64 * kRouteWaves)
topk_softmax_kernel(const float* __restrict__ logits, float* __restrict__ weights, int* __restrict__ indices,
                    const int64_t T, const int E, const int k, const int renorm) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * kRouteWaves + (threadIdx.x >> 6);
  if (t >= T) return;  // no workgroup barrier below
  route_topk_softmax_wave(logits + t * E, weights + t * k, indices + t * k, lane, E, k, renorm);
}

__global__ void __launch_bounds__(64 * kRouteWaves)
grouped_topk_sigmoid_kernel(const float* __restrict__ logits, const float* __restrict__ bias,
                            float* __restrict__ weights, int* __restrict__ indices, const int64_t T, const int E,
                            const int n_groups, const int topk_group, const int k, const float scaling) {
  __shared__ GroupedSmem sm;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  int64_t t = (int64_t)blockIdx.x * kRouteWaves + wv;
  const bool live = t < T;
  if (!live) t = T - 1;  // duplicate work, never stored: every wave reaches the barriers
  route_grouped_sigmoid_wave(logits + t * E, bias, sm, wv, weights + t * k, indices + t * k, live, lane, E, n_groups,
                             topk_group, k, scaling);
}

// ---- align ------------------------------------------------------------------------------------
// Every workgroup builds the same histogram and padded offsets (integer LDS atomics: exact, whatever
// the order), then each of its waves lays out ONE expert: it walks topk_ids in order and compacts the
// matching flat indices with a ballot, which gives the ascending order without any sorting pass, and
// fills the expert's padding.  E * n_flat index reads in total, all from L2: the arrays are tiny.
constexpr int kAlignThreads = 256;
constexpr int kAlignWaves = kAlignThreads / 64;

__global__ void __launch_bounds__(kAlignThreads)
align_block_kernel(const int* __restrict__ ids, int* __restrict__ sorted, int* __restrict__ expert_ids,
                   int* __restrict__ n_padded, int* __restrict__ cu_sum, const int n_flat, const int E,
                   const int bs_shift) {
  __shared__ int cnt[kMaxAlignExperts];
  __shared__ int off[kMaxAlignExperts + 1];
  __shared__ int tsum[kAlignThreads];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int bs = 1 << bs_shift;
  for (int e = tid; e < kMaxAlignExperts; e += kAlignThreads) cnt[e] = 0;
  __syncthreads();
  for (int i = tid; i < n_flat; i += kAlignThreads) {
    const int e = ids[i];
    if (e >= 0 && e < E) atomicAdd(&cnt[e], 1);
  }
  __syncthreads();
  // exclusive scan of the padded counts: thread t owns experts 4t .. 4t + 3
  int pc[4], local = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid * 4 + q;
    pc[q] = e < E ? ((cnt[e] + bs - 1) >> bs_shift) << bs_shift : 0;
    local += pc[q];
  }
  tsum[tid] = local;
  __syncthreads();
  for (int d = 1; d < kAlignThreads; d <<= 1) {
    const int v = tid >= d ? tsum[tid - d] : 0;
    __syncthreads();
    tsum[tid] += v;
    __syncthreads();
  }
  int run = tsum[tid] - local;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid * 4 + q;
    if (e < E) off[e] = run;
    run += pc[q];
  }
  if (tid == kAlignThreads - 1) off[E] = tsum[tid];  // experts >= E add nothing: the total
  __syncthreads();
  if (blockIdx.x == 0) {
    if (tid == 0) n_padded[0] = off[E];
    if (cu_sum)
      for (int e = tid; e <= E; e += kAlignThreads) cu_sum[e] = off[e];
  }
  const int e = blockIdx.x * kAlignWaves + (tid >> 6);
  if (e >= E) return;
  const int begin = off[e], end = off[e + 1];
  if (begin == end) return;  // empty expert: no block
  for (int b = (begin >> bs_shift) + lane; b < (end >> bs_shift); b += 64) expert_ids[b] = e;
  int pos = begin;
  for (int base = 0; base < n_flat; base += 64) {
    const int i = base + lane;
    const bool hit = i < n_flat && ids[i] == e;
    const unsigned long long mask = __ballot(hit);
    if (hit) sorted[pos + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    pos += __popcll(mask);
  }
  for (int p = pos + lane; p < end; p += 64) sorted[p] = n_flat;  // padding id
}

// ---- sum over the k expert outputs of a token ---------------------------------------------------
// addend (slm_moe_sum_add; nullptr in slm_moe_sum): one more [T, dim] row per token, added after slot k - 1 -- what
// slot k of a [T, k + 1, dim] input would be
template <typename T>
__global__ void __launch_bounds__(256)
moe_sum_kernel(uint16_t* __restrict__ out, const uint16_t* __restrict__ in, const uint16_t* __restrict__ addend,
               const int k, const int64_t dim) {
  const int64_t t = blockIdx.y;
  const uint16_t* src = in + t * k * dim;
  const uint16_t* add = addend ? addend + t * dim : nullptr;
  uint16_t* dst = out + t * dim;
  if ((dim & 7) == 0) {  // 16-byte pieces (rows are then 16-byte aligned: the bases are checked on the host)
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v * 8 >= dim) return;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(src + j * dim + v * 8);
      acc[0] += lo_f32<T>(w.x); acc[1] += hi_f32<T>(w.x); acc[2] += lo_f32<T>(w.y); acc[3] += hi_f32<T>(w.y);
      acc[4] += lo_f32<T>(w.z); acc[5] += hi_f32<T>(w.z); acc[6] += lo_f32<T>(w.w); acc[7] += hi_f32<T>(w.w);
    }
    if (add) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(add + v * 8);
      acc[0] += lo_f32<T>(w.x); acc[1] += hi_f32<T>(w.x); acc[2] += lo_f32<T>(w.y); acc[3] += hi_f32<T>(w.y);
      acc[4] += lo_f32<T>(w.z); acc[5] += hi_f32<T>(w.z); acc[6] += lo_f32<T>(w.w); acc[7] += hi_f32<T>(w.w);
    }
    u32x4 r;
    r.x = pack2<T>(acc[0], acc[1]); r.y = pack2<T>(acc[2], acc[3]);
    r.z = pack2<T>(acc[4], acc[5]); r.w = pack2<T>(acc[6], acc[7]);
    *reinterpret_cast<u32x4*>(dst + v * 8) = r;
  } else {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < dim; d += (int64_t)gridDim.x * 256) {
      float acc = 0.f;
      for (int j = 0; j < k; ++j) acc += lo_f32<T>((uint32_t)src[j * dim + d]);
      if (add) acc += lo_f32<T>((uint32_t)add[d]);
      dst[d] = pack1<T>(acc);
    }
  }
}

int route_check(const float* logits, const float* weights, const int32_t* indices, int64_t T, int32_t E, int32_t k) {
  const int rc = route_shape_check(T, E, k);
  if (rc != SLM_OK) return rc;
  if (T > 0 && (!logits || !weights || !indices)) return SLM_ERR_INVALID_ARG;
  return SLM_OK;
}

bool align_shape_ok(int64_t n_flat, int32_t E, int32_t bs) {
  return n_flat >= 0 && n_flat < ((int64_t)1 << 31) - 256 && E >= 1 && E <= kMaxAlignExperts &&
         (bs == 16 || bs == 32 || bs == 64 || bs == 128 || bs == 256);
}

}  // namespace
}  // namespace slm

extern "C" {

SLM_API int slm_moe_topk_softmax(const float* logits, float* weights, int32_t* indices, int64_t n_tokens,
                                 int32_t n_experts, int32_t topk, int32_t renormalize, void* stream) {
  using namespace slm;
  const int rc = route_check(logits, weights, indices, n_tokens, n_experts, topk);
  if (rc != SLM_OK || n_tokens == 0) return rc;
  hip_clear_error();
  const unsigned grid = (unsigned)((n_tokens + kRouteWaves - 1) / kRouteWaves);
  hipLaunchKernelGGL(topk_softmax_kernel, dim3(grid), dim3(64 * kRouteWaves), 0, reinterpret_cast<hipStream_t>(stream),
                     logits, weights, indices, n_tokens, n_experts, topk, renormalize);
  return hip_check_launch();
}

SLM_API int slm_moe_grouped_topk_sigmoid(const float* logits, const float* correction_bias, float* weights,
                                         int32_t* indices, int64_t n_tokens, int32_t n_experts,
                                         int32_t n_expert_groups, int32_t topk_group, int32_t topk,
                                         float scaling_factor, void* stream) {
  using namespace slm;
  const int rc = route_check(logits, weights, indices, n_tokens, n_experts, topk);
  if (rc != SLM_OK) return rc;
  if (route_groups_check(n_experts, n_expert_groups, topk_group, topk) != SLM_OK) return SLM_ERR_INVALID_ARG;
  if (n_tokens == 0) return SLM_OK;
  if (!correction_bias) return SLM_ERR_INVALID_ARG;
  hip_clear_error();
  const unsigned grid = (unsigned)((n_tokens + kRouteWaves - 1) / kRouteWaves);
  hipLaunchKernelGGL(grouped_topk_sigmoid_kernel, dim3(grid), dim3(64 * kRouteWaves), 0,
                     reinterpret_cast<hipStream_t>(stream), logits, correction_bias, weights, indices, n_tokens,
                     n_experts, n_expert_groups, topk_group, topk, scaling_factor);
  return hip_check_launch();
}

SLM_API int slm_moe_align_capacity(int64_t n_flat, int32_t n_experts, int32_t block_size, int64_t* max_padded,
                                   int64_t* max_blocks) {
  if (!slm::align_shape_ok(n_flat, n_experts, block_size)) return SLM_ERR_INVALID_ARG;
  const int64_t m = n_flat < n_experts ? n_flat : n_experts;  // experts that can be non-empty
  const int64_t blocks = (n_flat + m * (block_size - 1)) / block_size;
  if (max_padded) *max_padded = blocks * block_size;
  if (max_blocks) *max_blocks = blocks;
  return SLM_OK;
}

SLM_API int slm_moe_align_block(const slm_moe_align_args* a, void* stream) {
  using namespace slm;
  if (!a || !align_shape_ok(a->n_flat, a->n_experts, a->block_size)) return SLM_ERR_INVALID_ARG;
  if (!a->sorted_token_idxes || !a->expert_ids || !a->n_padded_tokens || (a->n_flat > 0 && !a->topk_ids))
    return SLM_ERR_INVALID_ARG;
  int64_t max_padded = 0, max_blocks = 0;
  (void)slm_moe_align_capacity(a->n_flat, a->n_experts, a->block_size, &max_padded, &max_blocks);
  if (a->sorted_capacity < max_padded || a->blocks_capacity < max_blocks) return SLM_ERR_INVALID_ARG;
  hip_clear_error();
  const unsigned grid = (unsigned)((a->n_experts + kAlignWaves - 1) / kAlignWaves);
  hipLaunchKernelGGL(align_block_kernel, dim3(grid), dim3(kAlignThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     a->topk_ids, a->sorted_token_idxes, a->expert_ids, a->n_padded_tokens, a->cu_sum,
                     (int)a->n_flat, a->n_experts, ilog2(a->block_size));
  return hip_check_launch();
}

static int moe_sum_launch(void* out, const void* in, const void* addend, int64_t n_tokens, int32_t topk, int64_t dim,
                          int32_t dtype, void* stream) {
  using namespace slm;
  if (n_tokens < 0 || topk < 1 || dim < 1) return SLM_ERR_INVALID_ARG;
  if (dtype != SLM_F16 && dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (n_tokens == 0) return SLM_OK;
  if (!out || !in || n_tokens > 65535 * (int64_t)32768) return SLM_ERR_INVALID_ARG;
  if ((dim & 7) == 0 && (!aligned16(out) || !aligned16(in) || !aligned16(addend))) return SLM_ERR_ALIGNMENT;
  hip_clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // blockIdx.y carries the token (<= 65535 per launch); x: 16-byte pieces, or a grid-stride loop over elements
  const int64_t xb = (dim & 7) == 0 ? (dim / 8 + 255) / 256 : (dim + 255) / 256;
  const unsigned gx = (unsigned)((dim & 7) != 0 && xb > 1024 ? 1024 : xb);
  for (int64_t t0 = 0; t0 < n_tokens; t0 += 65535) {
    const unsigned gy = (unsigned)(n_tokens - t0 < 65535 ? n_tokens - t0 : 65535);
    uint16_t* o = reinterpret_cast<uint16_t*>(out) + t0 * dim;
    const uint16_t* i = reinterpret_cast<const uint16_t*>(in) + t0 * topk * dim;
    const uint16_t* ad = addend ? reinterpret_cast<const uint16_t*>(addend) + t0 * dim : nullptr;
    if (dtype == SLM_BF16)
      hipLaunchKernelGGL(moe_sum_kernel<bf16_tag>, dim3(gx, gy), dim3(256), 0, st, o, i, ad, topk, dim);
    else
      hipLaunchKernelGGL(moe_sum_kernel<f16_tag>, dim3(gx, gy), dim3(256), 0, st, o, i, ad, topk, dim);
  }
  return hip_check_launch();
}

SLM_API int slm_moe_sum(void* out, const void* in, int64_t n_tokens, int32_t topk, int64_t dim, int32_t dtype,
                        void* stream) {
  return moe_sum_launch(out, in, nullptr, n_tokens, topk, dim, dtype, stream);
}

SLM_API int slm_moe_sum_add(void* out, const void* in, const void* addend, int64_t n_tokens, int32_t topk,
                            int64_t dim, int32_t dtype, void* stream) {
  if (n_tokens > 0 && topk >= 1 && dim >= 1 && (dtype == SLM_F16 || dtype == SLM_BF16) && !addend)
    return SLM_ERR_INVALID_ARG;
  return moe_sum_launch(out, in, addend, n_tokens, topk, dim, dtype, stream);
}

}  // extern "C"
