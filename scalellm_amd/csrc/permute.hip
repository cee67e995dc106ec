// permute.hip -- mixture-of-experts token permutation (include/slm_hip.h section 14):
//   slm_permute_index_map + slm_permute_rows   <- llm::kernel::moe::permute_with_index_map
//   slm_unpermute_rows                         <- llm::kernel::moe::unpermute_with_index_map / _with_mask_map
//   slm_permute_mask_map  + slm_permute_rows   <- llm::kernel::moe::permute_with_mask_map
//                                                 (moe/permutation_index_kernel.cu, permutation_mask_kernel.cu)
// One map convention for both forms: row_id_map [n_maps, n_tokens] int32, entry = row of the permuted tensor or -1.
// The map kernels are one launch each and pure functions of their input: every workgroup counts all assignments
// (integer LDS atomics: exact, whatever the order), scans the counts, and each of its waves places ONE expert by
// walking the input in order with a ballot -- the stable placement of slm_moe_align_block (moe.hip) without its
// padding.  The row kernels give one wave a 4 KiB segment of one token's row.
#include <type_traits>

#include "common.h"

namespace slm {
namespace {

struct f32_tag {};

constexpr int kMaxPermuteExperts = 1024;  // the limit of section 10 (slm_moe_align_block)
constexpr int kMapThreads = 256;
constexpr int kMapWaves = kMapThreads / 64;

// ---- maps -------------------------------------------------------------------------------------
// off[0 .. E]: exclusive scan of cnt[0 .. E); thread t owns experts 4t .. 4t + 3
__device__ __forceinline__ void exclusive_offsets(const int* cnt, int* off, int* tsum, const int E) {
  const int tid = threadIdx.x;
  int pc[4], local = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid * 4 + q;
    pc[q] = e < E ? cnt[e] : 0;
    local += pc[q];
  }
  tsum[tid] = local;
  __syncthreads();
  for (int d = 1; d < kMapThreads; d <<= 1) {
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
  if (tid == kMapThreads - 1) off[E] = tsum[tid];
  __syncthreads();
}

// kMask = false: src = topk_ids [T, n_maps] int32, map [n_maps, T]; within an expert ascending flat index t * k + j
// kMask = true:  src = routing_map [T, E] bytes (n_maps == E), map [E, T]; within an expert ascending token
// vec16: the mask may be counted in 16-byte pieces (its base is 16-byte aligned)
template <bool kMask>
__global__ void __launch_bounds__(kMapThreads)
permute_map_kernel(const void* __restrict__ src, int* __restrict__ map, int* __restrict__ tokens_per_expert,
                   int* __restrict__ n_permuted, const int T, const int n_maps, const int E, const int vec16) {
  __shared__ int cnt[kMaxPermuteExperts];
  __shared__ int off[kMaxPermuteExperts + 1];
  __shared__ int tsum[kMapThreads];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int* ids = reinterpret_cast<const int*>(src);
  const uint8_t* mask = reinterpret_cast<const uint8_t*>(src);
  const int n_flat = T * n_maps;  // < 2^31: checked on the host
  for (int e = tid; e < kMaxPermuteExperts; e += kMapThreads) cnt[e] = 0;
  __syncthreads();
  if constexpr (kMask) {
    const int nv = vec16 ? n_flat >> 4 : 0;
    for (int v = tid; v < nv; v += kMapThreads) {
      const u32x4 w = reinterpret_cast<const u32x4*>(mask)[v];
      if ((w.x | w.y | w.z | w.w) == 0u) continue;  // k of E bytes are set: most pieces are empty
      const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
      int e = (int)(((unsigned)v << 4) % (unsigned)E);
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        if ((ww[b >> 2] >> (8 * (b & 3))) & 0xffu) atomicAdd(&cnt[e], 1);
        e = e + 1 == E ? 0 : e + 1;
      }
    }
    for (int i = (nv << 4) + tid; i < n_flat; i += kMapThreads)
      if (mask[i]) atomicAdd(&cnt[i % E], 1);
  } else {
    for (int i = tid; i < n_flat; i += kMapThreads) {
      const int e = ids[i];
      if (e >= 0 && e < E) atomicAdd(&cnt[e], 1);
    }
  }
  __syncthreads();
  exclusive_offsets(cnt, off, tsum, E);
  if (blockIdx.x == 0) {
    if (tokens_per_expert)
      for (int e = tid; e < E; e += kMapThreads) tokens_per_expert[e] = cnt[e];
    if (n_permuted && tid == 0) n_permuted[0] = off[E];
    if constexpr (!kMask) {  // ids outside [0, E) take no row
      for (int i = tid; i < n_flat; i += kMapThreads) {
        const int e = ids[i];
        if (e < 0 || e >= E) {
          const int t = i / n_maps;
          map[(i - t * n_maps) * T + t] = -1;
        }
      }
    }
  }
  const int e = blockIdx.x * kMapWaves + (tid >> 6);
  if (e >= E) return;
  const bool any = cnt[e] > 0;  // the same in every lane of the wave
  int pos = off[e];
  if constexpr (kMask) {
    for (int base = 0; base < T; base += 64) {
      const int t = base + lane;
      const bool hit = any && t < T && mask[(int64_t)t * E + e] != 0;
      const unsigned long long m = __ballot(hit);
      if (t < T) map[(int64_t)e * T + t] = hit ? pos + __popcll(m & ((1ull << lane) - 1ull)) : -1;
      pos += __popcll(m);
    }
  } else {
    if (!any) return;
#pragma unroll 4
    for (int base = 0; base < n_flat; base += 64) {
      const int i = base + lane;
      const bool hit = i < n_flat && ids[i] == e;
      const unsigned long long m = __ballot(hit);
      if (hit) {
        const int t = i / n_maps;
        map[(i - t * n_maps) * T + t] = pos + __popcll(m & ((1ull << lane) - 1ull));
      }
      pos += __popcll(m);
    }
  }
}

// ---- rows -------------------------------------------------------------------------------------
// One wave per (token, segment): a segment is kSegVecs 16-byte vectors per lane = 4 KiB of the row, so a 16-bit row
// of 4096 is two waves and a 16-element row is one wave with a single live lane -- never a whole workgroup.
constexpr int kRowThreads = 256;
constexpr int kRowWaves = kRowThreads / 64;
constexpr int kSegVecs = 4;
constexpr int kSegSpan = 64 * kSegVecs;   // vectors of a row per segment
constexpr int64_t kMaxRowBlocks = 1 << 20;  // beyond it the waves loop

__device__ __forceinline__ int lane_value(const int v, const int src_lane) {
  return __builtin_amdgcn_readlane(v, src_lane);  // src_lane is wave-uniform at every call
}

// every source row is read once and stored to each of its mapped rows
__global__ void __launch_bounds__(kRowThreads)
permute_rows_kernel(u32x4* __restrict__ permuted, const u32x4* __restrict__ tokens, const int* __restrict__ map,
                    const int64_t T, const int n_maps, const int V, const int nseg, const int64_t permuted_rows) {
  const int lane = threadIdx.x & 63;
  const int64_t n_items = T * nseg;
  for (int64_t w = (int64_t)blockIdx.x * kRowWaves + (threadIdx.x >> 6); w < n_items;
       w += (int64_t)gridDim.x * kRowWaves) {
    const int64_t t = w / nseg;
    const int v0 = (int)(w - t * nseg) * kSegSpan + lane;
    u32x4 d[kSegVecs];
#pragma unroll
    for (int j = 0; j < kSegVecs; ++j)
      if (v0 + 64 * j < V) d[j] = tokens[t * V + v0 + 64 * j];
    for (int m0 = 0; m0 < n_maps; m0 += 64) {
      const int m = m0 + lane;
      const int row = m < n_maps ? map[(int64_t)m * T + t] : -1;
      unsigned long long live = __ballot(row >= 0 && row < permuted_rows);
      while (live) {
        const int b = __ffsll(live) - 1;
        live &= live - 1;
        u32x4* dst = permuted + (int64_t)lane_value(row, b) * V;
#pragma unroll
        for (int j = 0; j < kSegVecs; ++j)
          if (v0 + 64 * j < V) dst[v0 + 64 * j] = d[j];
      }
    }
  }
}

template <typename T>
struct Vec16 {
  static constexpr int n = std::is_same<T, f32_tag>::value ? 4 : 8;  // elements per 16-byte vector
};

template <typename T>
__device__ __forceinline__ void fma_vec(const float p, const u32x4 w, float* acc) {
  if constexpr (std::is_same<T, f32_tag>::value) {
    const f32x4 f = __builtin_bit_cast(f32x4, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(p, f[i], acc[i]);
  } else {
    const float f[8] = {lo_f32<T>(w.x), hi_f32<T>(w.x), lo_f32<T>(w.y), hi_f32<T>(w.y),
                        lo_f32<T>(w.z), hi_f32<T>(w.z), lo_f32<T>(w.w), hi_f32<T>(w.w)};
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(p, f[i], acc[i]);
  }
}

template <typename T>
__device__ __forceinline__ u32x4 round_vec(const float* acc) {
  if constexpr (std::is_same<T, f32_tag>::value) {
    const f32x4 f = {acc[0], acc[1], acc[2], acc[3]};
    return __builtin_bit_cast(u32x4, f);
  } else {
    u32x4 r;
    r.x = pack2<T>(acc[0], acc[1]); r.y = pack2<T>(acc[2], acc[3]);
    r.z = pack2<T>(acc[4], acc[5]); r.w = pack2<T>(acc[6], acc[7]);
    return r;
  }
}

template <typename P>
__device__ __forceinline__ float load_prob(const void* probs, const int64_t i) {
  if constexpr (std::is_same<P, f32_tag>::value) return reinterpret_cast<const float*>(probs)[i];
  else return lo_f32<P>((uint32_t) reinterpret_cast<const uint16_t*>(probs)[i]);
}

// out[t] = T(sum_m p[t, m] * permuted[map[m, t]]): fp32 fma chain in ascending m, one rounding (slm_moe_sum's
// convention; with p == 1 the fma IS its addition).  Two mapped rows are in flight at a time.
template <typename T, typename P>
__global__ void __launch_bounds__(kRowThreads)
unpermute_rows_kernel(u32x4* __restrict__ out, const u32x4* __restrict__ permuted, const int* __restrict__ map,
                      const void* __restrict__ probs, const int64_t n_tokens, const int n_maps, const int V,
                      const int nseg, const int64_t permuted_rows) {
  constexpr int kE = Vec16<T>::n;
  const int lane = threadIdx.x & 63;
  const int64_t n_items = n_tokens * nseg;
  for (int64_t w = (int64_t)blockIdx.x * kRowWaves + (threadIdx.x >> 6); w < n_items;
       w += (int64_t)gridDim.x * kRowWaves) {
    const int64_t t = w / nseg;
    const int v0 = (int)(w - t * nseg) * kSegSpan + lane;
    float acc[kSegVecs][kE];
#pragma unroll
    for (int j = 0; j < kSegVecs; ++j)
#pragma unroll
      for (int i = 0; i < kE; ++i) acc[j][i] = 0.f;
    for (int m0 = 0; m0 < n_maps; m0 += 64) {
      const int m = m0 + lane;
      const int row = m < n_maps ? map[(int64_t)m * n_tokens + t] : -1;
      const bool ok = row >= 0 && row < permuted_rows;
      const float p = probs && ok ? load_prob<P>(probs, t * n_maps + m) : 1.0f;
      const int pbits = __builtin_bit_cast(int, p);
      unsigned long long live = __ballot(ok);
      while (live) {
        const int b0 = __ffsll(live) - 1;
        live &= live - 1;
        const bool two = live != 0;
        const int b1 = two ? __ffsll(live) - 1 : b0;
        live &= live - 1;  // 0 stays 0
        const u32x4* s0 = permuted + (int64_t)lane_value(row, b0) * V;
        const u32x4* s1 = permuted + (int64_t)lane_value(row, b1) * V;
        const float p0 = __builtin_bit_cast(float, lane_value(pbits, b0));
        const float p1 = __builtin_bit_cast(float, lane_value(pbits, b1));
        u32x4 x0[kSegVecs], x1[kSegVecs];
#pragma unroll
        for (int j = 0; j < kSegVecs; ++j)
          if (v0 + 64 * j < V) {
            x0[j] = s0[v0 + 64 * j];
            if (two) x1[j] = s1[v0 + 64 * j];
          }
#pragma unroll
        for (int j = 0; j < kSegVecs; ++j)
          if (v0 + 64 * j < V) {
            fma_vec<T>(p0, x0[j], acc[j]);
            if (two) fma_vec<T>(p1, x1[j], acc[j]);
          }
      }
    }
#pragma unroll
    for (int j = 0; j < kSegVecs; ++j)
      if (v0 + 64 * j < V) out[t * V + v0 + 64 * j] = round_vec<T>(acc[j]);
  }
}

int elem_size(int32_t dtype) { return dtype == SLM_F32 ? 4 : (dtype == SLM_F16 || dtype == SLM_BF16) ? 2 : 0; }

// sizes shared by both row kernels; SLM_OK with *V == 0 never happens (dim >= 1)
int rows_check(int64_t n_tokens, int32_t n_maps, int64_t dim, int64_t permuted_rows, int32_t dtype, int* V) {
  if (n_tokens < 0 || n_maps < 1 || n_maps > kMaxPermuteExperts || dim < 1 || permuted_rows < 0)
    return SLM_ERR_INVALID_ARG;
  const int es = elem_size(dtype);
  if (es == 0 || (dim * es) % 16 != 0) return SLM_ERR_UNSUPPORTED;
  // rows are int32 in the map; a row's vectors and the map's entries are indexed in 32 bits per factor
  if (permuted_rows > 0x7fffffffll || dim * es / 16 > 0x7fffffll || n_tokens * n_maps >= ((int64_t)1 << 31) - 256)
    return SLM_ERR_INVALID_ARG;
  *V = (int)(dim * es / 16);
  return SLM_OK;
}

unsigned row_blocks(int64_t n_tokens, int nseg) {
  const int64_t b = (n_tokens * nseg + kRowWaves - 1) / kRowWaves;
  return (unsigned)(b < kMaxRowBlocks ? b : kMaxRowBlocks);
}

int map_check(const void* src, int64_t n_tokens, int32_t n_maps, int32_t n_experts, const int32_t* row_id_map) {
  if (n_tokens < 0 || n_maps < 1 || n_experts < 1 || n_experts > kMaxPermuteExperts ||
      n_tokens * n_maps >= ((int64_t)1 << 31) - 256)
    return SLM_ERR_INVALID_ARG;
  if (n_tokens > 0 && (!src || !row_id_map)) return SLM_ERR_INVALID_ARG;
  return SLM_OK;
}

}  // namespace
}  // namespace slm

extern "C" {

SLM_API int slm_permute_index_map(const int32_t* topk_ids, int64_t n_tokens, int32_t topk, int32_t n_experts,
                                  int32_t* row_id_map, int32_t* tokens_per_expert, void* stream) {
  using namespace slm;
  const int rc = map_check(topk_ids, n_tokens, topk, n_experts, row_id_map);
  if (rc != SLM_OK) return rc;
  if (n_tokens == 0 && !tokens_per_expert) return SLM_OK;  // nothing to write
  hip_clear_error();
  const unsigned grid = (unsigned)((n_experts + kMapWaves - 1) / kMapWaves);
  hipLaunchKernelGGL(permute_map_kernel<false>, dim3(grid), dim3(kMapThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), (const void*)topk_ids, row_id_map, tokens_per_expert,
                     (int*)nullptr, (int)n_tokens, topk, n_experts, 0);
  return hip_check_launch();
}

SLM_API int slm_permute_mask_map(const uint8_t* routing_map, int64_t n_tokens, int32_t n_experts,
                                 int32_t* row_id_map, int32_t* tokens_per_expert, int32_t* n_permuted, void* stream) {
  using namespace slm;
  const int rc = map_check(routing_map, n_tokens, n_experts, n_experts, row_id_map);
  if (rc != SLM_OK) return rc;
  if (n_tokens == 0 && !tokens_per_expert && !n_permuted) return SLM_OK;
  hip_clear_error();
  const unsigned grid = (unsigned)((n_experts + kMapWaves - 1) / kMapWaves);
  hipLaunchKernelGGL(permute_map_kernel<true>, dim3(grid), dim3(kMapThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), (const void*)routing_map, row_id_map, tokens_per_expert,
                     n_permuted, (int)n_tokens, n_experts, n_experts, aligned16(routing_map) ? 1 : 0);
  return hip_check_launch();
}

SLM_API int slm_permute_rows(void* permuted, const void* tokens, const int32_t* row_id_map, int64_t n_tokens,
                             int32_t n_maps, int64_t dim, int64_t permuted_rows, int32_t dtype, void* stream) {
  using namespace slm;
  int V = 0;
  const int rc = rows_check(n_tokens, n_maps, dim, permuted_rows, dtype, &V);
  if (rc != SLM_OK) return rc;
  if (n_tokens == 0 || permuted_rows == 0) return SLM_OK;  // no row to store
  if (!permuted || !tokens || !row_id_map) return SLM_ERR_INVALID_ARG;
  if (!aligned16(permuted) || !aligned16(tokens) || (reinterpret_cast<uintptr_t>(row_id_map) & 3u))
    return SLM_ERR_ALIGNMENT;
  hip_clear_error();
  const int nseg = (V + kSegSpan - 1) / kSegSpan;
  hipLaunchKernelGGL(permute_rows_kernel, dim3(row_blocks(n_tokens, nseg)), dim3(kRowThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<u32x4*>(permuted),
                     reinterpret_cast<const u32x4*>(tokens), row_id_map, n_tokens, n_maps, V, nseg, permuted_rows);
  return hip_check_launch();
}

SLM_API int slm_unpermute_rows(void* out, const void* permuted, const int32_t* row_id_map, const void* probs,
                               int32_t probs_dtype, int64_t n_tokens, int32_t n_maps, int64_t dim,
                               int64_t permuted_rows, int32_t dtype, void* stream) {
  using namespace slm;
  int V = 0;
  const int rc = rows_check(n_tokens, n_maps, dim, permuted_rows, dtype, &V);
  if (rc != SLM_OK) return rc;
  if (probs && probs_dtype != SLM_F32 && probs_dtype != dtype) return SLM_ERR_UNSUPPORTED;
  if (n_tokens == 0) return SLM_OK;
  if (!out || !row_id_map || (permuted_rows > 0 && !permuted)) return SLM_ERR_INVALID_ARG;
  const uintptr_t pmask = probs_dtype == SLM_F32 ? 3u : 1u;
  if (!aligned16(out) || !aligned16(permuted) || (reinterpret_cast<uintptr_t>(row_id_map) & 3u) ||
      (probs && (reinterpret_cast<uintptr_t>(probs) & pmask)))
    return SLM_ERR_ALIGNMENT;
  hip_clear_error();
  const int nseg = (V + kSegSpan - 1) / kSegSpan;
  const dim3 grid(row_blocks(n_tokens, nseg)), block(kRowThreads);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  u32x4* o = reinterpret_cast<u32x4*>(out);
  const u32x4* s = reinterpret_cast<const u32x4*>(permuted);
  const bool p32 = !probs || probs_dtype == SLM_F32;
#define SLM_UNPERMUTE(TT, PP)                                                                                  \
  hipLaunchKernelGGL((unpermute_rows_kernel<TT, PP>), grid, block, 0, st, o, s, row_id_map, probs, n_tokens, \
                     n_maps, V, nseg, permuted_rows)
  if (dtype == SLM_F32) SLM_UNPERMUTE(f32_tag, f32_tag);
  else if (dtype == SLM_BF16 && p32) SLM_UNPERMUTE(bf16_tag, f32_tag);
  else if (dtype == SLM_BF16) SLM_UNPERMUTE(bf16_tag, bf16_tag);
  else if (p32) SLM_UNPERMUTE(f16_tag, f32_tag);
  else SLM_UNPERMUTE(f16_tag, f16_tag);
#undef SLM_UNPERMUTE
  return hip_check_launch();
}

}  // extern "C"
