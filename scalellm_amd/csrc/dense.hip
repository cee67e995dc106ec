// dense.hip -- the weight-stream linears over checkpoint-layout weights, one kernel for all three weight sides:
//  * slm_linear (include/slm_hip.h section 13): unquantised f16 / bf16 weights; the reference's
//    {Column,Row}ParallelLinearImpl::forward = F::linear, src/layers/linear/parallel_linear.cpp:
//      C[M, N] = T( A[M, K] . W[N, K]^T + bias[N] )
//  * slm_fp8_linear (section 15): fp8 (e4m3fn) weight-only; the reference's marlin::fp8_gemm,
//    src/kernels/quantization/marlin.h:39-43, which reads a Marlin-repacked B -- this kernel reads the checkpoint
//    tensor as it is:
//      C[M, N] = T( (A[M, K] . e4m3(W[N, K])^T) * w_scale[N] + bias[N] )
//  * slm_mxfp4_linear (section 20): OCP MXFP4 weight-only (e2m1 nibbles, one e8m0 scale byte per 32 k), the Quark /
//    gpt-oss checkpoint tensors as they are:
//      C[M, N] = T( A[M, K] . T(e2m1(W[N, K]) * 2^(e[N, K/32] - 127))^T + bias[N] )
//
// The weight stream is moe_gemm.hip's: W[n, :] is k-contiguous and that IS an operand of the 32x32x16 MFMA
// (lane (n = lane & 31, h = lane >> 5) holds 8 consecutive k of row n), so the weights go from global memory
// to the MFMA in 16-B loads: no LDS stage, no transpose, no prepack.  K is streamed in 128-deep chunks, lane
// half h takes k = [64 h, 64 h + 64) of the chunk (contiguous bytes of row n); A's fragments come from a
// [rows][128 k] LDS image of the chunk in natural k order with w4_stream32.h's XOR swizzle.  A K that is no
// multiple of 128 ends in up to three 32-deep units in natural order.
//
// What differs from the grouped kernel:
//  * RT = 1 / 2 / 4 accumulator tiles of 32 rows per wave: every weight fragment feeds RT MFMAs, so the
//    weights are streamed once for M <= 32 RT.  More rows go to further row blocks of the grid (blockIdx.z),
//    which stream the weights again: correct, not tuned (prefill is not this kernel's job).
//  * the operands are swapped (weights = MFMA A, activations = MFMA B): the accumulator tile is C^T, lane
//    (m = lane & 31, h) holds for row m the columns 8 j + 4 h + {0..3} in registers 4 j .. 4 j + 3 -- four
//    consecutive columns, stored as ONE 16-B fp32 (slab) or 8-B T store.
//  * K split: blockIdx.y = slice s works on chunks [slice_chunk[s], slice_chunk[s + 1]) (the tail units go
//    with the last slice) and writes the fp32 slab s of [split_k][M][N] with plain stores; the reduce kernel
//    (or a deferred consumer: slm_rms_norm_splitk, slm_rope_kv_append_splitk, slm_gemma_norm) sums the slabs
//    with splitk_sum4 in slice order.  No atomics, no flags, no cross-workgroup hand-off.
//  * bias, and SiLU * mul over gate | up rows as in moe_gemm.hip (waves (0, 1) and (2, 3) hold the gate and
//    up tiles of one output tile; the up wave hands its T-rounded tile over through LDS).
//
// A workgroup is NW = 1 / 2 / 4 waves on adjacent column tiles sharing the A image; NW >= RT keeps the A
// ring at <= 8 16-B pieces per thread and chunk (the register budget of the three-chunk ring).  The host takes
// the narrowest NW that leaves at most two workgroups per CU; a wave's arithmetic does not depend on NW or RT.
// A partial last row tile clamps the row on load and suppresses the store; a partial NW group duplicates the
// last column tile and does not store it.
//
// Pipeline (moe_gemm.hip's): weights in a 3-chunk register ring, refilled right after their MFMAs; A in a
// 3-chunk register ring, written to the other LDS buffer one iteration before its use.  VMEM completes in
// order, so the A chunk that is waited for is two iterations old and the wait leaves two weight chunks in
// flight.  Loads past the slice's last chunk are clamped to it and never used.
//
// The weight side is the kernel parameter struct's compile-time choice (KP::SIDE: T / e4m3 / mxfp4); it sets:
//  * T weights: a lane's 64 k of a chunk are 128 bytes of row n, eight 16-B loads; load q IS the weight fragment
//    of MFMA step q.  A tail unit is two loads per lane half.
//  * e4m3 weights: the 64 k are 64 BYTES, four 16-B loads.  Load j holds k = 64 h + 16 j .. + 16, the fragments of
//    the two steps 2 j (dwords 0, 1) and 2 j + 1 (dwords 2, 3); a dword's low half is its lower k pair.  e4m3 -> T
//    is exact, two weights per v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0 (fp8_cvt.h): step q sees exactly
//    the k -- and the T values -- it sees on T(W), so under the same (RT, NW, split) the accumulators are the T
//    side's bit for bit.  A tail unit is one load per lane half.
//  * e4m3 only: y = acc * w_scale[n] in front of the epilogue (never the converter's scale operand), one fp32
//    multiply kept out of any contraction with the bias add; a K slice stores y into its slab, so the reduce kernel
//    and the deferred consumers see what a T call leaves.
//  * mxfp4 weights: the 64 k are 32 BYTES, two 16-B loads.  Load j is exactly one MX block (k = 64 h + 32 j .. + 32):
//    the fragments of the four steps 4 j .. 4 j + 3, one dword per step, a byte's low nibble the lower k.  The block's
//    scale byte w_scale[n, 4 c + 2 h + j] rides in the weight ring (two byte loads per lane and chunk: the scale row
//    stride carries no alignment; they are kept from merging into one 2-byte load, whose split the compiler schedules
//    with the load: that put a wait for the whole ring behind every refill) and goes into the converter as 2^(e - 127), four v_cvt_scalef32_pk_{bf16,f16}_fp4
//    per step (mxfp4_cvt.h).  e2m1 * 2^s is exact in T, so step q sees the T values it sees on T(dequant(W)) and the
//    accumulators are the T side's bit for bit; nothing is multiplied onto the accumulator.  A tail unit is one MX
//    block: ONE 8-B load per lane half (two steps) and the unit's scale byte.  Past a slice's last chunk the scale
//    index is clamped with the weight loads.
//
// Ring depth: LIN_RING = 3 chunks for the T and e4m3 sides and for the mxfp4 side but its one-wave form, although a
// chunk of e4m3 is half and one of mxfp4 a quarter of the bytes in flight.  It is the depth of BOTH register rings, and
// the A ring costs 4 P VGPRs a chunk (P = 8 RT / NW 16-B pieces per thread) beside the weight ring's 32, 16 or 10.  A
// six-chunk ring was built for the e4m3 forms with NW >= 2 RT (P <= 4; 264 VGPRs at RT 1 x NW 2, one wave per SIMD) and
// measured on gate_up: 33.8 / 38.4 us at M = 1 / 32 against 29.6 / 35.6 for three chunks
// (profiles/r17_fp8_ring_ab.jsonl), so it is not in the tree.  The mxfp4 side was measured at 3 / 4 / 6 / 8 chunks in
// every form (builds with -DSLM_LIN_MX_RING=R, tools/ab_mxfp4_ring.py, profiles/r22_mxfp4_ring_ab.jsonl): 6 and 8 lose
// on every row by 3-23 %; 4 wins 3-5 % on all six rows of the RT 1 x NW 1 form (qkv, o, down at M = 1 / 32: down
// 28.6 / 29.1 us against 29.7 / 30.1), ties or loses 0.5-4 % on the other forms (gate_up M = 32 32.6 against 32.0, down
// M = 128 35.0 against 33.5) except o at M = 128 (+ 2 %).  So the one-wave form, which has nothing else to hide a load
// behind, runs four chunks (LIN_MX_RING_1X1) and the others three.  No result bit depends on the depth (any depth >= 2:
// chunk i + 1 goes to LDS while chunk i is consumed): a wave's MFMAs run in chunk order.
#include <type_traits>

#include "common.h"
#include "dense_plan.h"
#include "fp8_cvt.h"
#include "mxfp4_cvt.h"
#include "tuning.h"

namespace slm {

constexpr int LIN_RING = 3;   // weight / A register rings (chunks)
constexpr int LIN_MX_RING_1X1 = 4;   // the mxfp4 side's one-wave form (RT 1 x NW 1), see "Ring depth" above
// -DSLM_LIN_MX_RING=R: every mxfp4 form at depth R >= 2, the build-time switch of tools/ab_mxfp4_ring.py

struct LinearKParams {
  static constexpr int SIDE = W_T;
  const char* a;
  const char* w;
  const void* bias;  // [N] T or NULL
  void* c;
  float* part;       // [split_k][M][N] or NULL (split_k == 1)
  int64_t lda, ldw, ldc;  // elements
  int M, N;
  int n_tiles;       // N / 32
  int tail_units;    // (K % 128) / 32
  int split_k;
  int silu;
  int slice_chunk[LIN_MAX_SPLIT + 1];
};

struct Fp8LinearKParams {
  static constexpr int SIDE = W_E4M3;
  const char* a;
  const char* w;
  const float* w_scale;  // [N] or NULL (1.0)
  const void* bias;      // [N] T or NULL
  void* c;
  float* part;           // [split_k][M][N] or NULL (split_k == 1)
  int64_t lda, ldw, ldc;  // elements (ldw: bytes)
  int M, N;
  int n_tiles;       // N / 32
  int tail_units;    // (K % 128) / 32
  int split_k;
  int silu;
  int slice_chunk[LIN_MAX_SPLIT + 1];
};

struct Mxfp4LinearKParams {
  static constexpr int SIDE = W_MXFP4;
  const char* a;
  const char* w;
  const uint8_t* w_scale;  // [N, K / 32] e8m0 bytes, row stride lds
  const void* bias;        // [N] T or NULL
  void* c;
  float* part;             // [split_k][M][N] or NULL (split_k == 1)
  int64_t lda, ldw, ldc;   // elements (ldw: bytes)
  int64_t lds;             // bytes
  int M, N;
  int n_tiles;       // N / 32
  int tail_units;    // (K % 128) / 32
  int split_k;
  int silu;
  int slice_chunk[LIN_MAX_SPLIT + 1];
};

template <typename T, int RT, int NW, typename KP>
__global__ void __launch_bounds__(NW * 64) linear_kernel(const KP p) {
  typedef typename Mfma<T>::frag frag_t;
  constexpr int SIDE = KP::SIDE;
  constexpr bool FP8 = SIDE == W_E4M3;
  constexpr bool MX = SIDE == W_MXFP4;
  constexpr int CB = SIDE == W_T ? 256 : FP8 ? 128 : 64;  // bytes of a 128-deep chunk of a weight row
  constexpr int WROW = SIDE == W_T ? 2 : 1;               // bytes per unit of ldw
  constexpr int WL = CB / 32;      // 16-B weight loads per lane and chunk
  constexpr int SPL = 8 / WL;      // MFMA steps (8 k) a 16-B weight load holds
#ifdef SLM_LIN_MX_RING
  constexpr int RING = MX ? SLM_LIN_MX_RING : LIN_RING;
#else
  constexpr int RING = MX && RT == 1 && NW == 1 ? LIN_MX_RING_1X1 : LIN_RING;
#endif
  static_assert(RING >= 2, "chunk i + 1 is stored to LDS while chunk i is consumed");
  constexpr int NT = NW * 64;
  constexpr int ROWS = RT * 32;
  constexpr int STAGE = ROWS * 256;  // one chunk of A: ROWS x 128 k
  constexpr int P = ROWS * 16 / NT;  // 16-B pieces of a chunk of A per thread
  static_assert(P >= 1 && P <= 8, "NW >= RT");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nb = blockIdx.x, ks = blockIdx.y;
  const int row0 = blockIdx.z * ROWS;

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

  // ---- the slice's chunks ----
  const int c0 = p.slice_chunk[ks];
  const int nC = p.slice_chunk[ks + 1] - c0;
  const int tail_units = ks == p.split_k - 1 ? p.tail_units : 0;
  const uint32_t a_kbase = (uint32_t)c0 * 256u;         // bytes into a row of A
  const uint32_t w_kbase = (uint32_t)c0 * (uint32_t)CB;  // bytes into a row of W

  // ---- A: this thread's P (row, 16-B slot) sources of a chunk; rows beyond M are clamped, never stored ----
  const char* a_src[P];
  int a_dst[P];
  const int a_slot = tid & 15;  // NT % 16 == 0: one slot for all of a thread's pieces
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int idx = tid + NT * i;
    const int row = idx >> 4, slot = idx & 15;
    int gr = row0 + row;
    gr = gr < p.M ? gr : p.M - 1;
    a_src[i] = p.a + 2 * ((int64_t)gr * p.lda + slot * 8) + a_kbase;
    a_dst[i] = stage_swz(row, slot);
  }
  const char* wlane = p.w + WROW * (((int64_t)nt * 32 + mrow) * p.ldw) + w_kbase;
  // mxfp4: the scale bytes of row n from the slice's first block on (four blocks per chunk)
  const uint8_t* slane = nullptr;
  const uint8_t* slane1 = nullptr;  // slane + 1, opaque
  if constexpr (MX) {
    slane = p.w_scale + ((int64_t)nt * 32 + mrow) * p.lds + (uint32_t)c0 * 4u;
    uint32_t one = 1;
    asm("" : "+s"(one));  // (an opaque OFFSET: the pointer keeps its global address space)
    slane1 = slane + one;
  }
  const int a_row = mrow * 256;
  const int a_swz = mrow & 15;

  f32x16 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

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
      for (int i = 0; i < P; ++i) *reinterpret_cast<u32x4*>(smem + stage * STAGE + a_dst[i]) = src[i];
    };
    // lane half kh: the CB / 2 contiguous bytes [kh * CB / 2, kh * CB / 2 + CB / 2) of the chunk's CB bytes of row n
    const char* wl = wlane + kh * (CB / 2);
    auto w_load = [&](int c, u32x4 (&w)[WL], uint32_t (&s)[2]) {
      const uint32_t cc = (uint32_t)clampc(c);
      const uint32_t off = cc * (uint32_t)CB;
#pragma unroll
      for (int j = 0; j < WL; ++j) w[j] = *reinterpret_cast<const u32x4*>(wl + off + j * 16);
      // blocks 4 c + 2 kh + {0, 1}: TWO byte loads (the row stride carries no alignment).  The second goes through
      // slane1, whose relation to slane the compiler does not know: merged into one 2-byte load, the split of the
      // pair is scheduled with the load and puts a wait for the whole ring behind every refill
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
          const char* sbase = smem + stage * STAGE + a_row;
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
#pragma unroll
              for (int t = 0; t < RT; ++t) {
                const frag_t af = __builtin_bit_cast(
                    frag_t, *reinterpret_cast<const u32x4*>(sbase + t * (32 * 256) + (((kh * 8 + q) ^ a_swz) << 4)));
                acc[t] = Mfma<T>::run(wf, af, acc[t]);
              }
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

  // ---- K % 128 (last slice): up to three 32-deep units in natural k order, one at a time ----
  if (tail_units > 0) {
    const uint32_t a_koff = (uint32_t)nC * 256u;  // bytes of a row of A behind the slice's chunks
    __syncthreads();                              // nobody reads the stages any more
#pragma unroll
    for (int i = 0; i < P; ++i) {
      if (a_slot < tail_units * 4)
        *reinterpret_cast<u32x4*>(smem + a_dst[i]) = *reinterpret_cast<const u32x4*>(a_src[i] + a_koff);
    }
    __syncthreads();
    const char* sbase = smem + a_row;
    // lane half kh: k = 16 kh .. + 16 of a unit (CB / 4 bytes of row n): CB / 8 bytes, TL 16-B loads -- mxfp4: ONE
    // 8-B load, the unit is one MX block with one scale byte
    constexpr int TL = MX ? 1 : CB / 128;
    const char* wt = wlane + (uint32_t)nC * (uint32_t)CB + kh * (CB / 8);
#pragma unroll
    for (int t3 = 0; t3 < 3; ++t3) {
      if (t3 < tail_units) {
        if constexpr (MX) {
          const u32x2 wv = *reinterpret_cast<const u32x2*>(wt + t3 * (CB / 4));
          const float bs = e8m0_scale(slane[(uint32_t)nC * 4u + t3]);
#pragma unroll
          for (int s = 0; s < 2; ++s) {  // step s of the unit: k = 16 kh + 8 s .. + 8
            const frag_t wf = fp4x8_frag<T>(s ? wv.y : wv.x, bs);
#pragma unroll
            for (int t = 0; t < RT; ++t) {
              const frag_t af = __builtin_bit_cast(
                  frag_t, *reinterpret_cast<const u32x4*>(sbase + t * (32 * 256) + (((t3 * 4 + kh * 2 + s) ^ a_swz) << 4)));
              acc[t] = Mfma<T>::run(wf, af, acc[t]);
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < TL; ++j) {
            const u32x4 wv = *reinterpret_cast<const u32x4*>(wt + t3 * (CB / 4) + j * 16);
#pragma unroll
            for (int h = 0; h < SPL; ++h) {
              const int s = j * SPL + h;  // step s of the unit: k = 16 kh + 8 s .. + 8
              const frag_t wf = step_frag<T, FP8>(wv, h);
#pragma unroll
              for (int t = 0; t < RT; ++t) {
                const frag_t af = __builtin_bit_cast(
                    frag_t, *reinterpret_cast<const u32x4*>(sbase + t * (32 * 256) + (((t3 * 4 + kh * 2 + s) ^ a_swz) << 4)));
                acc[t] = Mfma<T>::run(wf, af, acc[t]);
              }
            }
          }
        }
      }
    }
    __syncthreads();  // the SiLU exchange below reuses the stage
  }

  // ---- epilogue.  C^T layout: lane (m = lane & 31, kh), registers 4 j .. 4 j + 3 = columns 8 j + 4 kh + {0..3}
  const int ncol0 = nt * 32 + 4 * kh;  // + 8 j
  if constexpr (FP8) {  // y = acc * w_scale[n], in place
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 s = {1.f, 1.f, 1.f, 1.f};
      if (p.w_scale) s = *reinterpret_cast<const f32x4*>(p.w_scale + ncol0 + 8 * j);
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        acc[t][4 * j] = scaled(acc[t][4 * j], s.x);
        acc[t][4 * j + 1] = scaled(acc[t][4 * j + 1], s.y);
        acc[t][4 * j + 2] = scaled(acc[t][4 * j + 2], s.z);
        acc[t][4 * j + 3] = scaled(acc[t][4 * j + 3], s.w);
      }
    }
  }
  if (p.part) {  // a K slice: the fp32 slab, no bias, no rounding
    if (!nvalid) return;
    float* slab = p.part + (int64_t)ks * p.M * p.N;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int gm = row0 + t * 32 + mrow;
      if (gm < p.M) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 v = {acc[t][4 * j], acc[t][4 * j + 1], acc[t][4 * j + 2], acc[t][4 * j + 3]};
          *reinterpret_cast<f32x4*>(slab + (int64_t)gm * p.N + ncol0 + 8 * j) = v;
        }
      }
    }
    return;
  }
  // T( acc + bias ), packed pairs
  u32x2 packed[RT][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) {
      const u32x2 bv = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(p.bias) + ncol0 + 8 * j);
      b.x = lo_f32<T>(bv.x); b.y = hi_f32<T>(bv.x); b.z = lo_f32<T>(bv.y); b.w = hi_f32<T>(bv.y);
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      packed[t][j].x = pack2<T>(acc[t][4 * j] + b.x, acc[t][4 * j + 1] + b.y);
      packed[t][j].y = pack2<T>(acc[t][4 * j + 2] + b.z, acc[t][4 * j + 3] + b.w);
    }
  }
  uint16_t* cbase = reinterpret_cast<uint16_t*>(p.c);
  if constexpr (NW >= 2) {
    if (p.silu) {
      // the up wave hands its T-rounded tiles to the gate wave through the (now idle) A buffers; same lane, same (t, j)
      u32x2* ex = reinterpret_cast<u32x2*>(smem) + (wave >> 1) * (RT * 4 * 64);
      if (wave & 1) {
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int j = 0; j < 4; ++j) ex[(t * 4 + j) * 64 + lane] = packed[t][j];
      }
      __syncthreads();
      if ((wave & 1) || !nvalid) return;
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const int gm = row0 + t * 32 + mrow;
        if (gm < p.M) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const u32x2 g = packed[t][j], u = ex[(t * 4 + j) * 64 + lane];
            u32x2 r;
            r.x = pack2<T>(silu_mul1(lo_f32<T>(g.x), lo_f32<T>(u.x)), silu_mul1(hi_f32<T>(g.x), hi_f32<T>(u.x)));
            r.y = pack2<T>(silu_mul1(lo_f32<T>(g.y), lo_f32<T>(u.y)), silu_mul1(hi_f32<T>(g.y), hi_f32<T>(u.y)));
            // the gate wave: nt = the output tile
            *reinterpret_cast<u32x2*>(cbase + (int64_t)gm * p.ldc + ncol0 + 8 * j) = r;
          }
        }
      }
      return;
    }
  }
  if (!nvalid) return;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int gm = row0 + t * 32 + mrow;
    if (gm < p.M) {
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<u32x2*>(cbase + (int64_t)gm * p.ldc + ncol0 + 8 * j) = packed[t][j];
    }
  }
}

// ---- host: one path for slm_linear_args, slm_fp8_linear_args and slm_mxfp4_linear_args ----
template <typename T, int RT, int NW, typename KP>
static void launch_linear(const KP& kp, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((linear_kernel<T, RT, NW, KP>), grid, dim3(NW * 64), 0, st, kp);
}

template <typename T, typename KP>
static void launch_linear_form(const KP& kp, int rt, int nw, dim3 grid, hipStream_t st) {
  if (rt == 4) launch_linear<T, 4, 4>(kp, grid, st);
  else if (rt == 2 && nw == 4) launch_linear<T, 2, 4>(kp, grid, st);
  else if (rt == 2) launch_linear<T, 2, 2>(kp, grid, st);
  else if (nw == 4) launch_linear<T, 1, 4>(kp, grid, st);
  else if (nw == 2) launch_linear<T, 1, 2>(kp, grid, st);
  else launch_linear<T, 1, 1>(kp, grid, st);
}

template <typename Args>
static int linear_plan_info(const Args* a, slm_linear_plan_info* out) {
  LinearPlan pl;
  if (!out) return SLM_ERR_INVALID_ARG;
  const int rc = plan_linear(a, &pl);
  if (rc != SLM_OK) return rc;
  *out = slm_linear_plan_info{};
  out->row_tiles = pl.rt; out->waves = pl.nw;
  out->row_blocks = (int32_t)pl.row_blocks; out->col_groups = (int32_t)pl.col_groups;
  out->split_k = pl.split_k; out->n_chunks = pl.n_chunks; out->tail_units = pl.tail_units;
  for (int j = 0; j <= LIN_MAX_SPLIT; ++j) out->slice_chunk[j] = pl.slice_chunk[j];
  out->lds_bytes = pl.lds_bytes; out->workspace_bytes = pl.ws_bytes;
  return SLM_OK;
}

template <typename Args>
static size_t linear_workspace_bytes(const Args* a) {
  LinearPlan pl;
  return plan_linear(a, &pl) == SLM_OK ? (size_t)pl.ws_bytes : 0;
}

template <typename Args>
static int32_t linear_deferred_splits(const Args* a) {
  LinearPlan pl;
  return plan_linear(a, &pl) == SLM_OK && (a->flags & SLM_LINEAR_DEFER_REDUCE) && !a->bias && pl.split_k > 1
             ? pl.split_k : 0;
}

template <typename Args>
static int run_linear(const Args* a, void* stream) {
  constexpr bool FP8 = std::is_same<Args, slm_fp8_linear_args>::value;
  constexpr bool MX = std::is_same<Args, slm_mxfp4_linear_args>::value;
  LinearPlan pl;
  const int rc = plan_linear(a, &pl);
  if (rc != SLM_OK) return rc;
  if (a->M == 0) return SLM_OK;
  const bool silu = (a->flags & SLM_LINEAR_SILU_MUL) != 0;
  const bool defer = (a->flags & SLM_LINEAR_DEFER_REDUCE) && !a->bias && pl.split_k > 1;
  if (!a->a || !a->w || !a->c) return SLM_ERR_INVALID_ARG;
  // ldw counts T, e4m3 bytes or -- mxfp4 -- bytes of two weights
  if (a->lda < a->K || a->ldw < (MX ? a->K / 2 : a->K) || a->ldc < (silu ? a->N / 2 : a->N)) return SLM_ERR_INVALID_ARG;
  if constexpr (MX) {
    if (!a->w_scale || a->lds < a->K / 32) return SLM_ERR_INVALID_ARG;
  }
  // a weight row starts on a 16-B boundary: 8 T, 16 e4m3 or 32 e2m1 weights
  if (!aligned16(a->a) || a->lda % 8 || !aligned16(a->w) || a->ldw % (FP8 || MX ? 16 : 8) || !aligned16(a->c) ||
      a->ldc % 8 || (reinterpret_cast<uintptr_t>(a->bias) & 7u) || !aligned16(a->workspace))
    return SLM_ERR_ALIGNMENT;
  if constexpr (FP8) {
    if (!aligned16(a->w_scale)) return SLM_ERR_ALIGNMENT;
  }
  if (pl.ws_bytes > 0 && (!a->workspace || a->workspace_bytes < pl.ws_bytes)) return SLM_ERR_WORKSPACE;

  typename std::conditional<MX, Mxfp4LinearKParams,
                            typename std::conditional<FP8, Fp8LinearKParams, LinearKParams>::type>::type kp;
  kp.a = reinterpret_cast<const char*>(a->a);
  kp.w = reinterpret_cast<const char*>(a->w);
  if constexpr (FP8) kp.w_scale = a->w_scale;
  if constexpr (MX) { kp.w_scale = a->w_scale; kp.lds = a->lds; }
  kp.bias = pl.split_k > 1 ? nullptr : a->bias;  // a split call adds it in the reduce
  kp.c = a->c;
  kp.part = pl.split_k > 1 ? reinterpret_cast<float*>(a->workspace) : nullptr;
  kp.lda = a->lda; kp.ldw = a->ldw; kp.ldc = a->ldc;
  kp.M = (int)a->M; kp.N = (int)a->N;
  kp.n_tiles = (int)(a->N / 32);
  kp.tail_units = pl.tail_units;
  kp.split_k = pl.split_k;
  kp.silu = silu ? 1 : 0;
  for (int j = 0; j <= LIN_MAX_SPLIT; ++j) kp.slice_chunk[j] = pl.slice_chunk[j];
  hip_clear_error();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)pl.col_groups, (unsigned)pl.split_k, (unsigned)pl.row_blocks);
  dispatch_dtype(a->dtype, [&](auto t) { launch_linear_form<decltype(t)>(kp, pl.rt, pl.nw, grid, st); });
  int lrc = hip_check_launch();
  if (lrc != SLM_OK || pl.split_k == 1 || defer) return lrc;
  dispatch_dtype(a->dtype, [&](auto t) {
    launch_splitk_reduce<decltype(t)>(kp.part, a->bias, a->c, a->M, a->N, a->ldc, pl.split_k, st);
  });
  return hip_check_launch();
}

}  // namespace slm

extern "C" {

SLM_API int slm_linear_plan(const slm_linear_args* a, slm_linear_plan_info* out) {
  return slm::linear_plan_info(a, out);
}
SLM_API size_t slm_linear_workspace_bytes(const slm_linear_args* a) { return slm::linear_workspace_bytes(a); }
SLM_API int32_t slm_linear_deferred_splits(const slm_linear_args* a) { return slm::linear_deferred_splits(a); }
SLM_API int slm_linear(const slm_linear_args* a, void* stream) { return slm::run_linear(a, stream); }

SLM_API int slm_fp8_linear_plan(const slm_fp8_linear_args* a, slm_linear_plan_info* out) {
  return slm::linear_plan_info(a, out);
}
SLM_API size_t slm_fp8_linear_workspace_bytes(const slm_fp8_linear_args* a) { return slm::linear_workspace_bytes(a); }
SLM_API int32_t slm_fp8_linear_deferred_splits(const slm_fp8_linear_args* a) { return slm::linear_deferred_splits(a); }
SLM_API int slm_fp8_linear(const slm_fp8_linear_args* a, void* stream) { return slm::run_linear(a, stream); }

SLM_API int slm_mxfp4_linear_plan(const slm_mxfp4_linear_args* a, slm_linear_plan_info* out) {
  return slm::linear_plan_info(a, out);
}
SLM_API int32_t slm_mxfp4_linear_deferred_splits(const slm_mxfp4_linear_args* a) {
  return slm::linear_deferred_splits(a);
}
SLM_API int slm_mxfp4_linear(const slm_mxfp4_linear_args* a, void* stream) { return slm::run_linear(a, stream); }

}  // extern "C"
