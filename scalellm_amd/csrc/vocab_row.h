// vocab_row.h -- what the kernels that walk one vocabulary row per 1024-thread workgroup share (sampling.hip,
// rejection.hip; next to philox.h): the order-preserving key and the (key, ~index) composite every argmax is a
// max over, typed loads and stores, the wave and block reductions, and the radix select with the gather-and-sort
// of the top n.  The histogram word H is the includer's choice: uint32_t counts (rejection.hip: 1 KiB of bins),
// or 64-bit fixed-point masses (sampling.hip's top-p: 2 KiB).
//
// Include it BELOW `#pragma clang fp contract(off)`: the arithmetic here is part of what the includers promise
// to be plain IEEE fp32 (mass_q and the softmax numerator feed the top-p boundary).
#pragma once
#include <math.h>

#include "common.h"

namespace slm {
namespace vocab_row {  // the includers pull it into their own anonymous namespace

typedef unsigned long long u64;

constexpr int kThreads = 1024;  // one workgroup per row; thread t visits tokens t, t + 1024, ...
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kKeyNegInf = 0x007FFFFFu;  // f2key(-inf)
constexpr int kMaxVocab = 1 << 22;            // 2^22 tokens * 2^40 mass units < 2^64

// order-preserving key: larger key = larger value; -0 and +0 share one key (-0 + 0 = +0)
__device__ __forceinline__ uint32_t f2key(float x) {
  const uint32_t u = __float_as_uint(x + 0.0f);
  return u ^ ((u & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// (key desc, index asc) as one 64-bit max: ties go to the lower index whatever the reduction order
__device__ __forceinline__ u64 composite(float x, int i) {
  return ((u64)f2key(x) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)i);
}
__device__ __forceinline__ int composite_index(u64 c) { return (int)(0xFFFFFFFFu - (uint32_t)c); }

// softmax numerator and its fixed-point form in 2^-40 units (the top element weighs 2^40)
__device__ __forceinline__ float expm(float x, float m) { return expf(x - m); }
__device__ __forceinline__ u64 mass_q(float x, float m) {
  const float e = expm(x, m) * 1099511627776.0f;  // exact scaling by 2^40
  return e > 0.f ? (u64)e : 0ull;
}

template <int DT>
__device__ __forceinline__ float ld(const void* row, int i) {
  if constexpr (DT == SLM_F16) return (float)reinterpret_cast<const _Float16*>(row)[i];
  else if constexpr (DT == SLM_BF16)
    return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(row)[i] << 16);
  else return reinterpret_cast<const float*>(row)[i];
}
template <int DT>
__device__ __forceinline__ void st(void* row, int i, float x) {
  if constexpr (DT == SLM_F16) reinterpret_cast<_Float16*>(row)[i] = (_Float16)x;
  else if constexpr (DT == SLM_BF16) reinterpret_cast<uint16_t*>(row)[i] = pack1<bf16_tag>(x);
  else reinterpret_cast<float*>(row)[i] = x;
}
template <int DT>
constexpr int elem_bytes() { return DT == SLM_F32 ? 4 : 2; }

// what scan_bins publishes: the bin, the target inside it, the bin's weight.  Each width keeps the member order
// its kernel had: one 16-byte aligned (t, h) pair for 64-bit words, one 12-byte record for 32-bit ones.
template <class H>
struct RowSel {
  H t, h;
  uint32_t bin;
};
template <>
struct RowSel<uint32_t> {
  uint32_t bin, t, h;
};

// the LDS of the primitives below; a kernel that needs more derives from it
template <class H>
struct RowSmem {
  H hist[256];
  u64 red64[kWaves];
  float redf[kWaves];
  RowSel<H> sel;
  uint32_t top_key[SLM_SAMPLE_MAX_TOP];
  int32_t top_idx[SLM_SAMPLE_MAX_TOP];
  int32_t top_cnt;
};

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const u64 w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block max of a 64-bit composite (every thread gets it)
template <class S>
static __device__ u64 block_max_u64(u64 v, S& sm) {
  v = wave_max_u64(v);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) sm.red64[tid >> 6] = v;
  __syncthreads();
  u64 r = sm.red64[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) r = sm.red64[w] > r ? sm.red64[w] : r;
  __syncthreads();
  return r;
}
// block sum in a fixed order: thread-sequential, wave butterfly, waves in order
template <class S>
static __device__ float block_sum_f(float v, S& sm) {
  v = wave_sum_f(v);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) sm.redf[tid >> 6] = v;
  __syncthreads();
  float r = sm.redf[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) r += sm.redf[w];
  __syncthreads();
  return r;
}

// wave 0: find the bin b (scanning 255 -> 0) with before(b) <= t < before(b) + hist[b].
// frac >= 0 (64-bit masses only): t = floor(frac * total) (the top-p target, known once the first histogram is in).
template <class H>
static __device__ void scan_bins(RowSmem<H>& sm, H t, float frac) {
  const int lane = threadIdx.x;
  H h[4], s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { h[j] = sm.hist[255 - 4 * lane - j]; s += h[j]; }
  H inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const H n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  if constexpr (sizeof(H) == 8) {
    if (frac >= 0.f) {
      const u64 total = __shfl(inc, 63, 64);
      t = (u64)((double)frac * (double)total);
      if (t >= total) t = total - 1;
    }
  }
  H before = inc - s;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (before <= t && t < before + h[j]) {
      sm.sel.bin = 255 - 4 * lane - j;
      sm.sel.t = t - before;
      sm.sel.h = h[j];
    }
    before += h[j];
  }
}

struct Filter {
  uint32_t key;  // kept: key > this.key, or key == this.key and index <= imax
  int32_t imax;
  __device__ __forceinline__ bool keep(uint32_t k, int i) const { return k > key || (k == key && i <= imax); }
};

// Radix select over the order (key desc, index asc) of the eligible elements: the filter that keeps
// the element e with W(before e) <= t < W(before e) + w(e), and everything before it.
// elem(i, key, w) -> eligible; w = 1 (count) or the fixed-point mass (MASS: t = floor(frac * total), H = u64).
template <bool MASS, class H, class ElemF>
static __device__ Filter radix_select(const ElemF& elem, int V, H t, float frac, float m, RowSmem<H>& sm) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0, pmask = 0;
  H heq = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) sm.hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < V; i += kThreads) {
      uint32_t k;
      H w;
      if (elem(i, k, w) && w && (k & pmask) == prefix) atomicAdd(&sm.hist[(k >> shift) & 255u], w);
    }
    __syncthreads();
    if (tid < 64) scan_bins(sm, t, (MASS && shift == 24) ? frac : -1.f);
    __syncthreads();
    prefix |= sm.sel.bin << shift;
    pmask |= 255u << shift;
    t = sm.sel.t;
    heq = sm.sel.h;
    __syncthreads();  // sel_* are rewritten by the next pass
  }
  Filter f{prefix, 0x7FFFFFFF};
  H j = t, cnt = heq;  // position among the equal keys, their number
  if constexpr (MASS) {  // equal keys weigh the same: heq = cnt * q, the crossing is the j-th
    const u64 q = mass_q(key2f(prefix), m);
    if (q == 0) return f;  // a row without mass (non-finite logits): nothing to split
    cnt = heq / q;
    j = t / q;
  }
  if (j + 1 >= cnt) return f;
  // the (j + 1) lowest indices among the elements with key == prefix: select on inv = IM - i
  int nb = 1;
  while ((1 << nb) < V) ++nb;
  const uint32_t IM = (1u << nb) - 1u;
  uint32_t ip = 0, im = 0;
  for (int shift = ((nb - 1) / 8) * 8; shift >= 0; shift -= 8) {
    if (tid < 256) sm.hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < V; i += kThreads) {
      uint32_t k;
      H w;
      const uint32_t inv = IM - (uint32_t)i;
      if (elem(i, k, w) && w && k == prefix && (inv & im) == ip) atomicAdd(&sm.hist[(inv >> shift) & 255u], (H)1);
    }
    __syncthreads();
    if (tid < 64) scan_bins(sm, j, -1.f);
    __syncthreads();
    ip |= sm.sel.bin << shift;
    im |= 255u << shift;
    j = sm.sel.t;
    __syncthreads();
  }
  f.imax = (int32_t)(IM - ip);
  return f;
}

// the elements the filter keeps (n <= SLM_SAMPLE_MAX_TOP of them: a count-mode radix_select with t = n - 1) into
// sm.top_key / top_idx, sorted (key desc, index asc) by thread 0.  No barrier behind the sort: thread 0 may go on
// reading its own writes; other readers synchronise first.
template <class H, class ElemF>
static __device__ void gather_sort_top(const ElemF& elem, int V, int n, const Filter fn, RowSmem<H>& sm) {
  const int tid = threadIdx.x;
  if (tid == 0) sm.top_cnt = 0;
  __syncthreads();
  for (int i = tid; i < V; i += kThreads) {
    uint32_t k;
    H w;
    elem(i, k, w);
    if (fn.keep(k, i)) {
      const int slot = atomicAdd(&sm.top_cnt, 1);
      if (slot < SLM_SAMPLE_MAX_TOP) { sm.top_key[slot] = k; sm.top_idx[slot] = i; }
    }
  }
  __syncthreads();
  if (tid == 0) {
    for (int a = 1; a < n; ++a) {  // insertion sort: key desc, index asc
      const uint32_t k = sm.top_key[a];
      const int32_t ix = sm.top_idx[a];
      int b = a - 1;
      while (b >= 0 && (sm.top_key[b] < k || (sm.top_key[b] == k && sm.top_idx[b] > ix))) {
        sm.top_key[b + 1] = sm.top_key[b];
        sm.top_idx[b + 1] = sm.top_idx[b];
        --b;
      }
      sm.top_key[b + 1] = k;
      sm.top_idx[b + 1] = ix;
    }
  }
}

}  // namespace vocab_row
}  // namespace slm
