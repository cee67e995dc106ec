// moe_gemm.hip -- grouped GEMM over the experts of a mixture-of-experts layer, checkpoint-layout weights, one kernel
// for all three weight sides:
//  * slm_moe_gemm (include/slm_hip.h section 10): dense fp16 / bf16 experts; the reference's
//    Sm80KernelGroupedGemm, src/kernels/gemm/, in its own form: A[m, k], W[e, n, k], rows gathered through
//    sorted_token_idxes / expert_ids
//  * slm_moe_fp8_gemm (section 16): fp8 (e4m3fn) weight-only experts with fp32 channel scales
//  * slm_moe_mxfp4_gemm (section 21): OCP MXFP4 weight-only experts (e2m1 nibbles, one e8m0 scale byte per 32 k), the
//    Quark / gpt-oss checkpoint tensors as they are.
//
// For every 32-row block b of the aligned token list (slm_moe_align_block with block_size 32):
//     C[idx, :] = epilogue( A[idx / a_div, :] . W_e^T ),  e = expert_ids[b], idx = sorted[b * 32 + r]
// (e4m3: epilogue( (A . e4m3(W_e)^T) * w_scale[e, :] ); mxfp4: W_e = T(e2m1(W_e) * 2^(w_scale[e, n, k / 32] - 127))).
// The aligned-list contract is w4_moe.hip's; what differs is the weight operand.  W_e is the checkpoint
// tensor [N, K], k-contiguous, and that IS the B operand of the 32x32x16 MFMA: lane (n = lane & 31,
// h = lane >> 5) holds 8 consecutive k of column n.  So the weights go from global memory to the MFMA
// in 16-B loads: no LDS stage, no transpose, no prepack.
//
// k order.  An MFMA sums 16 products; which 16 k they are is free as long as both operands agree.  K is
// streamed in 128-deep chunks and lane half h takes the k range [64 h, 64 h + 64) of the chunk: its
// 16-B loads are contiguous bytes of row n (a cache line when ldw allows it), and MFMA step q = 0..7
// sums k = 64 h + 8 q + j over (h, j).  A's fragments come from a [32 rows][128 k] LDS image of the chunk
// in natural k order: lane (r, h) reads slot 8 h + q of row r (w4_stream32.h's XOR swizzle: conflict-free
// ds_read_b128).  A K that is no multiple of 128 ends in up to three 32-deep units in natural order
// (lane half h: k = 16 h + 8 s + j, s = 0, 1), staged and consumed one at a time.
//
// Decomposition.  One wave owns one 32 x 32 output tile over the whole K: a fixed accumulation order for
// every element, whatever the launch shape.  A workgroup is NW = 4, 2 or 1 waves on adjacent column tiles
// sharing the A image; the host takes the widest NW that still gives every CU a workgroup (moe_gemm_waves:
// a pure function of max_blocks, N and the flags, so repeats and graph replays stay bit-identical, and
// because a wave's arithmetic does not depend on NW the result is the same for every choice).  No split-K,
// no workspace, no atomics.
//
// Pipeline (the shape of w4_stream32.h): weights in a 3-chunk register ring, refilled right after their
// MFMAs; A in a 3-chunk register ring, written to the other LDS buffer one iteration before its use.  VMEM
// completes in order, so the A chunk that is waited for is two iterations old and the wait leaves two
// weight chunks in flight.  Loads past the last chunk are clamped to it and never used.
//
// SLM_MOE_SILU_MUL: rows [0, N/2) of W_e are the gate, [N/2, N) the up projection; waves (0, 1) and
// (2, 3) hold the (gate, up) tiles of one output tile, the up wave hands its T-rounded tile over through
// LDS: the bits of the plain GEMM followed by slm_silu_mul.
//
// The weight side is the kernel parameter struct's compile-time choice (KP::SIDE: T / e4m3 / mxfp4), as in dense.hip:
//  * T weights: a lane's 64 k of a chunk are 128 bytes of row n, eight 16-B loads; load q IS the weight fragment
//    of MFMA step q.  A tail unit is two loads per lane half.
//  * e4m3 weights: the 64 k are 64 BYTES, four 16-B loads; load j holds the fragments of the two steps 2 j (dwords
//    0, 1) and 2 j + 1 (dwords 2, 3).  e4m3 -> T is exact (fp8_cvt.h): step q sees exactly the k -- and the T
//    values -- it sees on T(W), so the accumulators are the T side's bit for bit.  A tail unit is one load per lane
//    half.
//  * e4m3 only, the scale.  In the C layout of the 32x32 MFMA a lane holds ONE column (col = lane & 31): one scale
//    load per lane, w_scale[e * scale_stride + n].  It multiplies the fp32 accumulator (never the converter's scale
//    operand), then row_scale[idx] multiplies that product, then one rounding.  Under SiLU * mul the gate and the
//    up wave each scale their tile by their own channels before the T rounding and the LDS hand-over.
//  * mxfp4 weights (dense.hip's mxfp4 side, lane for lane): the 64 k are 32 BYTES, two 16-B loads.  Load j is exactly
//    one MX block (k = 64 h + 32 j .. + 32): the fragments of the four steps 4 j .. 4 j + 3, one dword per step, a
//    byte's low nibble the lower k.  The block's scale byte w_scale[e, n, 4 c + 2 h + j] rides in the weight ring as
//    TWO byte loads per lane and chunk (the scale strides carry no alignment; dense.hip's header says why they are kept
//    from merging into one 2-byte load) and goes into the converter as 2^(e - 127), four
//    v_cvt_scalef32_pk_{bf16,f16}_fp4 per step (mxfp4_cvt.h).  e2m1 * 2^s is exact in T wherever it is a normal
//    number of T, so step q sees the T values it sees on T(dequant(W)) and the accumulators are the T side's bit for
//    bit; nothing is multiplied onto the accumulator, and the three epilogues are the T side's.  A tail unit is one MX
//    block: ONE 8-B load per lane half (two steps) and the unit's scale byte.
//    Addresses.  Row n = nt * 32 + (lane & 31) < N because nt is clamped to n_tiles - 1.  A ring load of chunk c reads
//    bytes [64 cc + 32 h + 16 j, + 16) of the row with cc = min(c, n_chunks - 1): below 64 n_chunks <= K / 2.  A tail
//    load reads [64 n_chunks + 16 t + 8 h, + 8) with t < tail_units: below 64 n_chunks + 16 tail_units = K / 2.  The
//    scale index is clamped by the SAME cc: 4 cc + 2 h + j <= 4 n_chunks - 1, and the tail's 4 n_chunks + t <
//    4 n_chunks + tail_units = K / 32.  The host checks ldw >= K / 2, lds >= K / 32 and both expert strides >=
//    (N - 1) * stride + row length, and the kernel leaves on an expert id outside [0, E) before it forms an address: no
//    load leaves expert e's own [N, K / 2] and [N, K / 32] rows, whatever the padding between them holds.
// Ring depth: MG_RING = 3 chunks for all three weight sides, as dense.hip found (its header: a six-chunk ring measured
// slower on e4m3, and on mxfp4 four chunks won only in the one-wave form of a kernel with up to four row tiles).  No
// result bit depends on it.
#include <type_traits>

#include "common.h"
#include "fp8_cvt.h"
#include "moe_gemm_plan.h"
#include "mxfp4_cvt.h"

namespace slm {

struct MoeDenseKParams {
  static constexpr int SIDE = W_T;
  const void* a;
  const char* w;            // expert 0
  void* c;
  const float* row_scale;   // [n_flat] or NULL
  const int32_t* sorted;    // [>= n_padded]
  const int32_t* expert_ids;
  const int32_t* n_padded;  // [1]
  int64_t w_stride;         // bytes per expert
  int64_t lda, ldw, ldc;    // elements
  int n_flat;               // rows of c; indices >= n_flat are padding
  int a_div;
  int n_experts;
  int n_tiles;              // N / 32
  int n_chunks;             // K / 128
  int tail_units;           // (K % 128) / 32
  int n_nblocks;            // workgroups per row block
  int silu;
};

struct MoeFp8KParams {
  static constexpr int SIDE = W_E4M3;
  const void* a;
  const char* w;            // expert 0
  const float* w_scale;     // expert 0's [N], or NULL (1.0)
  void* c;
  const float* row_scale;   // [n_flat] or NULL
  const int32_t* sorted;    // [>= n_padded]
  const int32_t* expert_ids;
  const int32_t* n_padded;  // [1]
  int64_t w_stride;         // bytes per expert
  int64_t scale_stride;     // floats per expert
  int64_t lda, ldw, ldc;    // elements (ldw: bytes)
  int n_flat;               // rows of c; indices >= n_flat are padding
  int a_div;
  int n_experts;
  int n_tiles;              // N / 32
  int n_chunks;             // K / 128
  int tail_units;           // (K % 128) / 32
  int n_nblocks;            // workgroups per row block
  int silu;
};

struct MoeMxfp4KParams {
  static constexpr int SIDE = W_MXFP4;
  const void* a;
  const char* w;            // expert 0
  const uint8_t* w_scale;   // expert 0's [N, K / 32] e8m0 bytes, row stride lds
  void* c;
  const float* row_scale;   // [n_flat] or NULL
  const int32_t* sorted;    // [>= n_padded]
  const int32_t* expert_ids;
  const int32_t* n_padded;  // [1]
  int64_t w_stride;         // bytes per expert
  int64_t scale_stride;     // scale bytes per expert
  int64_t lda, ldw, ldc;    // elements (ldw: bytes)
  int64_t lds;              // bytes
  int n_flat;               // rows of c; indices >= n_flat are padding
  int a_div;
  int n_experts;
  int n_tiles;              // N / 32
  int n_chunks;             // K / 128
  int tail_units;           // (K % 128) / 32
  int n_nblocks;            // workgroups per row block
  int silu;
};

template <typename T, int NW, typename KP>
__global__ void __launch_bounds__(NW * 64) moe_gemm_kernel(const KP p) {
  typedef typename Mfma<T>::frag frag_t;
  constexpr int SIDE = KP::SIDE;
  constexpr bool FP8 = SIDE == W_E4M3;
  constexpr bool MX = SIDE == W_MXFP4;
  constexpr int CB = SIDE == W_T ? 256 : FP8 ? 128 : 64;  // bytes of a 128-deep chunk of a weight row
  constexpr int WROW = SIDE == W_T ? 2 : 1;               // bytes per unit of ldw
  constexpr int WL = CB / 32;      // 16-B weight loads per lane and chunk
  constexpr int SPL = 8 / WL;      // MFMA steps (8 k) a 16-B weight load holds
#ifdef SLM_MG_MX_RING  // every mxfp4 form at depth R >= 2: the build-time switch of tools/ab_moe_mxfp4_ring.py
  constexpr int RING = MX ? SLM_MG_MX_RING : MG_RING;
#else
  constexpr int RING = MG_RING;
#endif
  static_assert(RING >= 2, "chunk i + 1 is stored to LDS while chunk i is consumed");
  constexpr int NT = NW * 64;
  constexpr int P = 512 / NT;  // 16-B pieces of a chunk of A per thread
  __shared__ __attribute__((aligned(16))) char smem[MG_LDS_BYTES];
  __shared__ int s_idx[32];  // the block's flat indices, for the scatter in the epilogue
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nb = blockIdx.x % p.n_nblocks;
  const int mb = blockIdx.x / p.n_nblocks;
  if ((int64_t)mb * 32 >= (int64_t)p.n_padded[0]) return;  // beyond the aligned list: nothing to do
  const int e = p.expert_ids[mb];
  if ((unsigned)e >= (unsigned)p.n_experts) return;        // never produced by the align step

  // ---- the wave's column tile ----
  int nt;
  bool nvalid;
  if (p.silu) {
    // pairs of waves: (gate, up) tiles of output tile pi
    const int half_tiles = p.n_tiles >> 1;
    int pi = nb * (NW / 2) + (wave >> 1);
    nvalid = pi < half_tiles;
    if (!nvalid) pi = half_tiles - 1;  // clamped duplicate work, never stored
    nt = (wave & 1) * half_tiles + pi;
  } else {
    nt = nb * NW + wave;
    nvalid = nt < p.n_tiles;
    if (!nvalid) nt = p.n_tiles - 1;
  }
  const int mrow = lane & 31, kh = lane >> 5;

  // ---- A: this thread's P (row, 16-B slot) sources of a chunk; the row comes from the sorted list ----
  const int32_t* blk = p.sorted + (int64_t)mb * 32;
  if (tid < 32) s_idx[tid] = blk[tid];
  const char* abase = reinterpret_cast<const char*>(p.a);
  const char* a_src[P];
  int a_dst[P];
  const int a_slot = tid & 15;  // NT % 16 == 0: one slot for all of a thread's pieces
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int idx = tid + NT * i;
    const int row = idx >> 4, slot = idx & 15;
    const int fi = blk[row];
    const int64_t ar = (unsigned)fi < (unsigned)p.n_flat ? fi / p.a_div : 0;  // padding: a clamped row
    a_src[i] = abase + 2 * (ar * p.lda + slot * 8);
    a_dst[i] = stage_swz(row, slot);
  }
  // the expert base is a 64-bit pointer, offsets inside an expert 32-bit
  const char* wexp = p.w + (int64_t)e * p.w_stride;
  // the lane's row of W_e = its column of C (clamped tiles: a valid duplicate)
  const int64_t ncol = (int64_t)nt * 32 + mrow;
  const char* wlane = wexp + WROW * (ncol * p.ldw);
  // mxfp4: the scale bytes of row n of expert e (four blocks per chunk)
  const uint8_t* slane = nullptr;
  const uint8_t* slane1 = nullptr;  // slane + 1, opaque
  if constexpr (MX) {
    slane = p.w_scale + (int64_t)e * p.scale_stride + ncol * p.lds;
    uint32_t one = 1;
    asm("" : "+s"(one));  // (an opaque OFFSET: the pointer keeps its global address space)
    slane1 = slane + one;
  }
  const int a_row = mrow * 256;
  const int a_swz = mrow & 15;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  const int nC = p.n_chunks;
  if (nC > 0) {
    const int last = nC - 1;
    auto clampc = [&](int c) { return c < last ? c : last; };
    u32x4 areg[RING][P];
    u32x4 wreg[RING][WL];
    // mxfp4 only: the e8m0 byte of load j's block, riding in the weight ring as the load leaves it (zero-extended);
    // 2^(e - 127) is made where the chunk is consumed, so no wait sits behind the refill
    uint32_t sreg[RING][2];
    auto a_load = [&](int c, u32x4 (&dst)[P]) {
      const uint32_t off = (uint32_t)clampc(c) * 256u;
#pragma unroll
      for (int i = 0; i < P; ++i) dst[i] = *reinterpret_cast<const u32x4*>(a_src[i] + off);
    };
    auto a_store = [&](int stage, const u32x4 (&src)[P]) {
#pragma unroll
      for (int i = 0; i < P; ++i) *reinterpret_cast<u32x4*>(smem + stage * MG_STAGE_BYTES + a_dst[i]) = src[i];
    };
    // lane half kh: the CB / 2 contiguous bytes [kh * CB / 2, kh * CB / 2 + CB / 2) of the chunk's CB bytes of row n
    const char* wl = wlane + kh * (CB / 2);
    auto w_load = [&](int c, u32x4 (&w)[WL], uint32_t (&s)[2]) {
      const uint32_t cc = (uint32_t)clampc(c);
      const uint32_t off = cc * (uint32_t)CB;
#pragma unroll
      for (int j = 0; j < WL; ++j) w[j] = *reinterpret_cast<const u32x4*>(wl + off + j * 16);
      // blocks 4 c + 2 kh + {0, 1}: TWO byte loads (dense.hip's header: merged into one 2-byte load, the split of
      // the pair is scheduled with the load and puts a wait for the whole ring behind every refill)
      if constexpr (MX) {
        s[0] = slane[cc * 4u + 2 * kh];
        s[1] = slane1[cc * 4u + 2 * kh];
      }
    };

    // prologue in the order the steady-state iterations issue (A, then the weights of the same chunk)
    a_load(0, areg[0]);
    w_load(0, wreg[0], sreg[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int d = 1; d < RING; ++d) {
      a_load(d, areg[d]);
      __builtin_amdgcn_sched_barrier(0);
      w_load(d, wreg[d], sreg[d]);
      __builtin_amdgcn_sched_barrier(0);
    }
    a_store(0, areg[0]);
    __syncthreads();

    int stage = 0;
    const int n_iter = (nC + RING - 1) / RING * RING;
    for (int base = 0; base < n_iter; base += RING) {
#pragma unroll
      for (int u = 0; u < RING; ++u) {
        const int i = base + u;  // chunk; ring slot u
        // A for chunk i + RING into the registers chunk i left (stored one iteration ago)
        a_load(i + RING, areg[u]);
        __builtin_amdgcn_sched_barrier(0);
        if (i < nC) {
          const char* sbase = smem + stage * MG_STAGE_BYTES + a_row;
#pragma unroll
          for (int j = 0; j < WL; ++j) {
            float bs = 1.f;  // mxfp4: 2^(e - 127) of load j's block, the converter's scale operand
            if constexpr (MX) bs = e8m0_scale(sreg[u][j]);
#pragma unroll
            for (int h = 0; h < SPL; ++h) {
              const int q = j * SPL + h;  // MFMA step q: k = 64 kh + 8 q .. + 8 of the chunk
              frag_t wf;
              if constexpr (MX) wf = fp4x8_frag<T>(wreg[u][j][h], bs);
              else wf = step_frag<T, FP8>(wreg[u][j], h);
              const frag_t af = __builtin_bit_cast(
                  frag_t, *reinterpret_cast<const u32x4*>(sbase + (((kh * 8 + q) ^ a_swz) << 4)));
              acc = Mfma<T>::run(af, wf, acc);
            }
          }
        }
        // the refill AFTER the old values are consumed (pinned): each ring slot keeps its registers
        __builtin_amdgcn_sched_barrier(0);
        w_load(i + RING, wreg[u], sreg[u]);
        __builtin_amdgcn_sched_barrier(0);
        // chunk i + 1 (loaded RING - 1 iterations ago) -> the buffer everybody finished reading one barrier ago
        a_store(stage ^ 1, areg[(u + 1) % RING]);
        __syncthreads();
        stage ^= 1;
      }
    }
  }

  // ---- K % 128: up to three 32-deep units in natural k order, one at a time ----
  if (p.tail_units > 0) {
    const uint32_t a_koff = (uint32_t)nC * 256u;  // bytes of a row of A behind the chunks
    __syncthreads();                              // nC == 0: s_idx; otherwise nobody reads the stages any more
#pragma unroll
    for (int i = 0; i < P; ++i) {
      if (a_slot < p.tail_units * 4)
        *reinterpret_cast<u32x4*>(smem + a_dst[i]) = *reinterpret_cast<const u32x4*>(a_src[i] + a_koff);
    }
    __syncthreads();
    const char* sbase = smem + a_row;
    // lane half kh: k = 16 kh .. + 16 of a unit (CB / 4 bytes of row n): CB / 8 bytes, TL 16-B loads -- mxfp4: ONE
    // 8-B load, the unit is one MX block with one scale byte
    constexpr int TL = MX ? 1 : CB / 128;
    const char* wt = wlane + (uint32_t)nC * (uint32_t)CB + kh * (CB / 8);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      if (t < p.tail_units) {
        if constexpr (MX) {
          const u32x2 wv = *reinterpret_cast<const u32x2*>(wt + t * (CB / 4));
          const float bs = e8m0_scale(slane[(uint32_t)nC * 4u + t]);
#pragma unroll
          for (int s = 0; s < 2; ++s) {  // step s of the unit: k = 16 kh + 8 s .. + 8
            const frag_t wf = fp4x8_frag<T>(s ? wv.y : wv.x, bs);
            const frag_t af = __builtin_bit_cast(
                frag_t, *reinterpret_cast<const u32x4*>(sbase + (((t * 4 + kh * 2 + s) ^ a_swz) << 4)));
            acc = Mfma<T>::run(af, wf, acc);
          }
        } else {
#pragma unroll
          for (int j = 0; j < TL; ++j) {
            const u32x4 wv = *reinterpret_cast<const u32x4*>(wt + t * (CB / 4) + j * 16);
#pragma unroll
            for (int h = 0; h < SPL; ++h) {
              const int s = j * SPL + h;  // step s of the unit: k = 16 kh + 8 s .. + 8
              const frag_t wf = step_frag<T, FP8>(wv, h);
              const frag_t af = __builtin_bit_cast(
                  frag_t, *reinterpret_cast<const u32x4*>(sbase + (((t * 4 + kh * 2 + s) ^ a_swz) << 4)));
              acc = Mfma<T>::run(af, wf, acc);
            }
          }
        }
      }
    }
    __syncthreads();  // the SiLU exchange below reuses the stage
  }

  if constexpr (FP8) {  // y = acc * w_scale[e, n]: the lane's one column, one fp32 multiply per element, in place
    if (p.w_scale) {
      const float s = p.w_scale[(int64_t)e * p.scale_stride + ncol];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = scaled(acc[r], s);
    }
  }

  // ---- epilogue: C/D layout of the 32x32 MFMA: col = lane & 31, row = (r&3) + 8*(r>>2) + 4*(lane>>5); the row goes to C[idx];
  // s_idx was written before the first barrier.  Kept local and written out: with the shared cd_store /
  // cd_silu_exchange of w4_epilogue.h the NW = 4 form took 5 VGPRs less, a third wave per SIMD, and measured 1.6 %
  // slower at 256 tokens
  uint16_t* cbase = reinterpret_cast<uint16_t*>(p.c);
  if constexpr (NW >= 2) {
    if (p.silu) {
      // the up wave hands its T-rounded tile to the gate wave through the (now idle) A buffers; same lane, same r
      uint16_t* ex = reinterpret_cast<uint16_t*>(smem) + (wave >> 1) * 1024;
      if (wave & 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) ex[r * 64 + lane] = pack1<T>(acc[r]);
      }
      __syncthreads();
      if ((wave & 1) || !nvalid) return;
#pragma unroll
      for (int r = 0; r < 16; ++r) {  // the gate wave: nt = the output tile, ncol the output column
        const int fi = s_idx[(r & 3) + 8 * (r >> 2) + 4 * kh];
        const float g = lo_f32<T>((uint32_t)pack1<T>(acc[r]));
        const float u = lo_f32<T>((uint32_t)ex[r * 64 + lane]);
        if ((unsigned)fi < (unsigned)p.n_flat) cbase[(int64_t)fi * p.ldc + ncol] = pack1<T>(silu_mul1(g, u));
      }
      return;
    }
  }
  if (!nvalid) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int fi = s_idx[(r & 3) + 8 * (r >> 2) + 4 * kh];
    if ((unsigned)fi < (unsigned)p.n_flat) {
      float v = acc[r];
      if (p.row_scale) v *= p.row_scale[fi];
      cbase[(int64_t)fi * p.ldc + ncol] = pack1<T>(v);
    }
  }
}

// ---- host: one path for slm_moe_gemm_dense_args, slm_moe_fp8_gemm_args and slm_moe_mxfp4_gemm_args ----
// (the launch shape, moe_gemm_waves, is moe_gemm_plan.h's)
template <typename T, int NW, typename KP>
static void launch_moe_gemm(const KP& kp, unsigned grid, hipStream_t st) {
  hipLaunchKernelGGL((moe_gemm_kernel<T, NW, KP>), dim3(grid), dim3(NW * 64), 0, st, kp);
}

template <typename T, typename KP>
static void launch_moe_gemm_nw(const KP& kp, int nw, unsigned grid, hipStream_t st) {
  if (nw == 4) launch_moe_gemm<T, 4>(kp, grid, st);
  else if (nw == 2) launch_moe_gemm<T, 2>(kp, grid, st);
  else launch_moe_gemm<T, 1>(kp, grid, st);
}

template <typename Args>
static int run_moe_gemm(const Args* a, void* stream) {
  constexpr bool FP8 = std::is_same<Args, slm_moe_fp8_gemm_args>::value;
  constexpr bool MX = std::is_same<Args, slm_moe_mxfp4_gemm_args>::value;
  // ldw and w_expert_stride count T, e4m3 bytes or -- mxfp4 -- bytes of two weights
  constexpr int WB = FP8 || MX ? 1 : 2;   // bytes per unit of ldw
  constexpr int WA = 16 / WB;             // units per 16-B load
  if (!a) return SLM_ERR_INVALID_ARG;
  if (a->n_flat < 0 || a->K <= 0 || a->N <= 0 || a->a_div < 1 || a->n_experts < 1 || a->max_blocks < 0)
    return SLM_ERR_INVALID_ARG;
  if (a->dtype != SLM_F16 && a->dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (a->flags & ~SLM_MOE_SILU_MUL) return SLM_ERR_INVALID_ARG;
  const bool silu = (a->flags & SLM_MOE_SILU_MUL) != 0;
  if (silu && a->row_scale) return SLM_ERR_INVALID_ARG;
  if (a->K % 32 || a->N % 32 || (silu && (a->N / 2) % 32)) return SLM_ERR_UNSUPPORTED;
  // 32-bit byte offsets inside one expert; flat indices are int32
  const int64_t krow = MX ? a->K / 2 : a->K;  // units of ldw in a weight row
  if (krow * a->N * WB >= ((int64_t)1 << 32) || a->n_flat >= ((int64_t)1 << 31) - 256) return SLM_ERR_UNSUPPORTED;
  if (a->n_flat == 0 || a->max_blocks == 0) return SLM_OK;
  if (!a->a || !a->w || !a->c || !a->sorted_token_idxes || !a->expert_ids || !a->n_padded_tokens)
    return SLM_ERR_INVALID_ARG;
  const int64_t n_out = silu ? a->N / 2 : a->N;
  if (a->lda < a->K || a->ldw < krow || a->ldc < n_out || a->w_expert_stride < (a->N - 1) * a->ldw + krow)
    return SLM_ERR_INVALID_ARG;
  if constexpr (FP8) {
    if (a->w_scale && a->w_scale_expert_stride < a->N) return SLM_ERR_INVALID_ARG;
  }
  if constexpr (MX) {  // one e8m0 byte per 32 k, required; no alignment of base or strides
    if (!a->w_scale || a->lds < a->K / 32 || a->w_scale_expert_stride < (a->N - 1) * a->lds + a->K / 32)
      return SLM_ERR_INVALID_ARG;
  }
  if (!aligned16(a->a) || a->lda % 8 || !aligned16(a->w) || a->ldw % WA || a->w_expert_stride % WA ||
      (reinterpret_cast<uintptr_t>(a->c) & 1u) || (reinterpret_cast<uintptr_t>(a->row_scale) & 3u))
    return SLM_ERR_ALIGNMENT;
  if constexpr (FP8) {
    if (reinterpret_cast<uintptr_t>(a->w_scale) & 3u) return SLM_ERR_ALIGNMENT;
  }
  if (a->N * a->ldw * WB >= ((int64_t)1 << 32)) return SLM_ERR_UNSUPPORTED;  // a strided expert: still < 4 GiB
  if constexpr (MX) {
    if (a->N * a->lds >= ((int64_t)1 << 32)) return SLM_ERR_UNSUPPORTED;
  }
  const int64_t n_tiles = a->N / 32;
  const int nw = moe_gemm_waves(a->max_blocks, n_tiles, silu);
  const int64_t n_nblocks = gemm_col_groups(n_tiles, nw, silu);
  const int64_t grid = (int64_t)a->max_blocks * n_nblocks;
  if (grid >= ((int64_t)1 << 31)) return SLM_ERR_UNSUPPORTED;

  typename std::conditional<MX, MoeMxfp4KParams,
                            typename std::conditional<FP8, MoeFp8KParams, MoeDenseKParams>::type>::type kp;
  kp.a = a->a;
  kp.w = reinterpret_cast<const char*>(a->w);
  kp.c = a->c;
  kp.row_scale = a->row_scale;
  kp.sorted = a->sorted_token_idxes;
  kp.expert_ids = a->expert_ids;
  kp.n_padded = a->n_padded_tokens;
  kp.w_stride = a->w_expert_stride * WB;
  if constexpr (FP8) {
    kp.w_scale = a->w_scale;
    kp.scale_stride = a->w_scale ? a->w_scale_expert_stride : 0;
  }
  if constexpr (MX) {
    kp.w_scale = a->w_scale;
    kp.scale_stride = a->w_scale_expert_stride;
    kp.lds = a->lds;
  }
  kp.lda = a->lda; kp.ldw = a->ldw; kp.ldc = a->ldc;
  kp.n_flat = (int)a->n_flat;
  kp.a_div = a->a_div;
  kp.n_experts = a->n_experts;
  kp.n_tiles = (int)n_tiles;
  kp.n_chunks = (int)(a->K / MG_KC);
  kp.tail_units = (int)((a->K % MG_KC) / 32);
  kp.n_nblocks = (int)n_nblocks;
  kp.silu = silu ? 1 : 0;
  hip_clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dispatch_dtype(a->dtype, [&](auto t) { launch_moe_gemm_nw<decltype(t)>(kp, nw, (unsigned)grid, st); });
  return hip_check_launch();
}

}  // namespace slm

extern "C" {

SLM_API int slm_moe_gemm(const slm_moe_gemm_dense_args* a, void* stream) { return slm::run_moe_gemm(a, stream); }
SLM_API int slm_moe_fp8_gemm(const slm_moe_fp8_gemm_args* a, void* stream) { return slm::run_moe_gemm(a, stream); }
SLM_API int slm_moe_mxfp4_gemm(const slm_moe_mxfp4_gemm_args* a, void* stream) { return slm::run_moe_gemm(a, stream); }

}  // extern "C"
