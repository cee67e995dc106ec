// philox.h -- the counter-based RNG of the sampling entry points (include/slm_hip.h sections 8 and 9).
//
// Philox4x32-10 (Salmon et al., SC'11; the constants of Random123, rocRAND and torch).
// key (seed lo, seed hi); counter (lo32(i >> 2), hi32(i >> 2), pos, stream); token i takes word i & 3,
// so one 10-round block serves the 4 consecutive ids 4q .. 4q + 3.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace slm {

struct PhiloxBlock {
  uint32_t w[4];
};

// the block of ids 4q .. 4q + 3 (q < 2^30: hi32(q) = 0)
__device__ __forceinline__ PhiloxBlock philox_block(unsigned long long seed, uint32_t pos, uint32_t stream,
                                                    uint32_t q) {
  uint32_t c0 = q, c1 = 0u, c2 = pos, c3 = stream;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int rnd = 0; rnd < 10; ++rnd) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return PhiloxBlock{{c0, c1, c2, c3}};
}

// the word of id i alone (a whole block per word: use philox_block where 4 consecutive ids are drawn)
__device__ __forceinline__ uint32_t philox_word(unsigned long long seed, uint32_t pos, uint32_t stream, uint32_t i) {
  const PhiloxBlock b = philox_block(seed, pos, stream, i >> 2);
  const uint32_t w = i & 3u;
  return w == 0 ? b.w[0] : w == 1 ? b.w[1] : w == 2 ? b.w[2] : b.w[3];
}

// u = ((x >> 8) + 0.5) 2^-24 in (0, 1), exact in fp32
__device__ __forceinline__ float uniform24(uint32_t x) { return ((float)(x >> 8) + 0.5f) * 0x1p-24f; }

// E = -ln(u), u = ((x >> 8) + 0.5) 2^-24 in (0, 1): from u itself below 1/2, from 1 - u above
// (both exact in fp32, so E never rounds to 0 and keeps its precision next to u = 1)
__device__ __forceinline__ float exp_draw(uint32_t x) {
  const uint32_t m = x >> 8;
  if (m < (1u << 23)) return -logf(((float)m + 0.5f) * 0x1p-24f);
  return -log1pf(-(((float)((1u << 24) - 1u - m) + 0.5f) * 0x1p-24f));
}

}  // namespace slm
