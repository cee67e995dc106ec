// w4_stream32.h -- the 32-row weight-stream main loop of the lean int4 kernels: one 32 x 32 output tile per
// wave, K streamed in 128-deep chunks.  Two kernels run it and differ only in what surrounds it:
//   w4_small.hip  dense rows m0 .. m0 + 31, split-K bounds, bias / split-K / SiLU epilogue
//   w4_moe.hip    rows gathered through an expert's sorted index list, scatter / row_scale / SiLU epilogue
// (the MoE instance is the one that serves production decode).
//
// Everything ordering-sensitive lives here and only here: the A staging ring, the weight / scale ring, the
// prologue pinned with sched_barriers, and the eight-step unpack / MFMA / post-scale loop (why post-scaled,
// why no LDS-DMA, why a 4-chunk ring: w4_small.hip's header).
#pragma once
#include "w4_common.h"

namespace slm {

constexpr int S32_STAGES = 2;          // A tile buffers
constexpr int S32_STAGE_BYTES = 32 * 256;
constexpr int S32_RING = 4;            // weight ring (chunks)
constexpr size_t S32_LDS_BYTES = S32_STAGES * S32_STAGE_BYTES;

// A chunk's A tile is 32 rows x 16 slots of 16 B (8 k-values); thread tid stages the two (row, slot) pairs
// idx = tid + 256 * i, row = idx >> 4, slot = idx & 15: the caller turns the row into a source pointer and
// takes the byte offset inside a stage buffer from common.h's stage_swz (XOR swizzle: conflict-free
// ds_read_b128 fragments).
//
// Streams chunks [c0, c1) (c1 > c0) and returns the wave's 32 x 32 accumulator tile in the C/D layout of
// the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
//   a_src[i]  this thread's two A source pointers at chunk 0 (16 B each per chunk, + 256 B per chunk)
//   a_dst[i]  stage_swz of the same two (row, slot) pairs
//   smem      S32_LDS_BYTES of dynamic LDS; free for the caller's epilogue after the return (the last
//             iteration ends in a barrier)
//   wlane / szlane  per-lane bases of the wave's column tile in the packed weights / the scale table
//   wstride   bytes per 64-deep half chunk; szstride  bytes per scale group
//   cpg_shift log2(chunks per scale group) (NG == 1)
//   mrow, kh  lane & 31 and lane >> 5, formed ONCE in the caller, which needs them for its epilogue too.  The
//             compiler simplifies caller and callee separately before it inlines this function: derived again
//             in here they are different expressions to it, the kernel gets other address arithmetic and
//             another register assignment through the whole loop; in that form the dense gate_up GEMM
//             measured 2.3-2.8 % slower than before the extraction (profiles/r11_refactor_codegen.md).  The chunk range comes as [c0, c1), not as a
//             count, for the same reason.
// NG: scale groups per 128-deep chunk (1 for group >= 128, 2 for 64, 4 for 32)
// SPAN: scale groups wider than a chunk (group 256.., per-channel): group boundaries are tested at
//       run time; the common group sizes keep every accumulate/epilogue decision static
template <typename T, int NG, bool SPAN>
__device__ __forceinline__ f32x16 w4_stream32(char* smem, const char* const (&a_src)[2], const int (&a_dst)[2],
                                              const char* wlane, const char* szlane, const uint32_t wstride,
                                              const uint32_t szstride, const int cpg_shift, const int c0,
                                              const int c1, const int mrow, const int kh) {
  typedef typename Mfma<T>::frag frag_t;
  constexpr int WPG = 8 / NG;  // k-steps (words) per scale group within a chunk
  const int nC = c1 - c0;  // >= 1
  const int last = c1 - 1;
  auto clampc = [&](int c) { return c < last ? c : last; };

  // ---- A staging: global loads, swizzled LDS writes ----
  // chunk c lives in areg[c % S32_RING] from its load (iteration c-4) to its LDS store (iteration
  // c-1).  The long residence is deliberate: VMEM completes in order, so waiting for an A load
  // also waits for every weight load issued before it -- an A load only one iteration old would
  // cap the weight ring at two chunks in flight; a three-iterations-old one costs nothing.
  u32x4 areg[S32_RING][2];
  auto a_load = [&](int c, u32x4 (&dst)[2]) {
    const uint32_t off = (uint32_t)clampc(c) * 256u;  // < 2 GiB: checked on the host
#pragma unroll
    for (int i = 0; i < 2; ++i) dst[i] = *reinterpret_cast<const u32x4*>(a_src[i] + off);
  };
  auto a_store = [&](int stage, const u32x4 (&src)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      *reinterpret_cast<u32x4*>(smem + stage * S32_STAGE_BYTES + a_dst[i]) = src[i];
  };

  // ---- weight / scale rings ----
  u32x4 wreg[S32_RING][2];
  uint32_t szreg[S32_RING][NG];
  // the per-lane bases are computed once by the caller; per load only a wave-uniform 32-bit byte offset is
  // added (the host checks that the packed weights and the scale table are < 4 GiB): scalar address math is
  // issue slots too
  auto w_load = [&](int c, u32x4 (&w)[2], uint32_t (&sz)[NG]) {
    const uint32_t cc = (uint32_t)clampc(c);
#pragma unroll
    for (int h = 0; h < 2; ++h)
      w[h] = __builtin_nontemporal_load(
          reinterpret_cast<const u32x4*>(wlane + (cc * 2 + h) * wstride));
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const uint32_t grp = NG > 1 ? cc * NG + g : (cc >> cpg_shift);
      sz[g] = *reinterpret_cast<const uint32_t*>(szlane + grp * szstride);
    }
  };

  // prologue in the ORDER the steady-state iterations issue (iteration k: A for chunk k+4, then
  // the refill = weights for chunk k+4), so the compiler's counted waits hold from iteration 0
  a_load(c0, areg[0]);
  w_load(c0, wreg[0], szreg[0]);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int d = 1; d < S32_RING; ++d) {
    a_load(c0 + d, areg[d]);
    __builtin_amdgcn_sched_barrier(0);
    w_load(c0 + d, wreg[d], szreg[d]);
    __builtin_amdgcn_sched_barrier(0);
  }
  a_store(0, areg[0]);

  f32x16 acc, tmp, tmpx;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = tmp[r] = tmpx[r] = 0.f;
  const u32x4 ones4 = {W4Ones<T>::bits, W4Ones<T>::bits, W4Ones<T>::bits, W4Ones<T>::bits};
  const frag_t ones = __builtin_bit_cast(frag_t, ones4);
  uint32_t magic_v = W4Magic<T>::bits;
  asm volatile("" : "+v"(magic_v));  // keep it in a VGPR (not re-materialised as a literal)
  uint32_t mask_s = 0x000F000Fu;
  asm volatile("" : "+s"(mask_s));   // ... and the nibble-pair mask in an SGPR
  const int a_row = mrow * 256;
  const int a_swz = mrow & 15;

  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

  bool group_open = false;  // tmp / tmpx hold a partial group (groups wider than a chunk)
  int stage = 0;
  const int n_iter = (nC + S32_RING - 1) / S32_RING * S32_RING;
  for (int base = 0; base < n_iter; base += S32_RING) {
#pragma unroll
    for (int u = 0; u < S32_RING; ++u) {
      const int i = base + u;  // chunk (relative); ring slot u
      // A for chunk i+4 into the registers chunk i left (stored one iteration ago)
      a_load(c0 + i + S32_RING, areg[u]);
      __builtin_amdgcn_sched_barrier(0);
      if (i < nC) {
        const char* sbase = smem + stage * S32_STAGE_BYTES + a_row;
        // does the scale group that ends this chunk end HERE (groups >= 128 may span chunks)
        const int cabs = c0 + i;
        const bool grp_ends = !SPAN || i == nC - 1 || ((cabs + 1) >> cpg_shift) != (cabs >> cpg_shift);
        frag_t af = __builtin_bit_cast(
            frag_t, *reinterpret_cast<const u32x4*>(sbase + (((0 * 2 + kh) ^ a_swz) << 4)));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          frag_t af_n = af;
          if (j < 7)
            af_n = __builtin_bit_cast(
                frag_t, *reinterpret_cast<const u32x4*>(sbase + ((((j + 1) * 2 + kh) ^ a_swz) << 4)));
          const u32x4 wv = wreg[u][j >> 2];
          const uint32_t word = (j & 3) == 0 ? wv.x : (j & 3) == 1 ? wv.y : (j & 3) == 2 ? wv.z : wv.w;
          uint32_t o[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            // (x & mask) | magic in ONE VALU op, v_and_or_b32: VOP3 takes no literals on gfx9-family,
            // so the mask rides in an SGPR and the magic in a VGPR, both opaque to the optimiser (with
            // literals hipcc emits v_and + v_or).  A plain expression, NOT inline asm: hipcc inserts
            // no hazard wait states behind an asm statement, and an MFMA issued right behind an asm
            // v_and_or_b32 reads stale B operands (seen in round 2 with independent MFMA chains).
            const uint32_t x = q == 0 ? word : word >> (4 * q);
            o[q] = (x & mask_s) | magic_v;
          }
          const u32x4 packed = {o[0], o[1], o[2], o[3]};
          const frag_t bf = __builtin_bit_cast(frag_t, packed);
          const bool g_first = (j % WPG) == 0 && !(SPAN && group_open);
          if (g_first) {
            f32x16 z;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = 0.f;
            tmp = Mfma<T>::run(af, bf, z);
            tmpx = Mfma<T>::run(af, ones, z);
          } else {
            tmp = Mfma<T>::run(af, bf, tmp);
            tmpx = Mfma<T>::run(af, ones, tmpx);
          }
          const bool g_last = (j % WPG) == WPG - 1;
          if (g_last && (!SPAN || grp_ends)) {
            // acc += s * (tmp - (magic + z) * X) for this lane's column
            float sc, zm;
            W4Magic<T>::decode(szreg[u][j / WPG], sc, zm);
            const float nzs = -zm * sc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = fmaf(sc, tmp[r], fmaf(nzs, tmpx[r], acc[r]));
          }
          af = af_n;
        }
        if constexpr (SPAN) group_open = !grp_ends;
      }
      // refills AFTER the old values are consumed (pinned): each ring slot keeps its registers
      __builtin_amdgcn_sched_barrier(0);
      w_load(c0 + i + S32_RING, wreg[u], szreg[u]);
      __builtin_amdgcn_sched_barrier(0);
      // chunk i+1 (loaded three iterations ago; counted wait: three and a half iterations of
      // loads stay in flight) -> the buffer everybody finished reading one barrier ago
      a_store(stage ^ 1, areg[(u + 1) % S32_RING]);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      stage ^= 1;
    }
  }
  return acc;
}

}  // namespace slm
