// w4.hip -- int4-weight x fp16/bf16-activation GEMM for gfx950 (CDNA4): prepack, dequant, GEMM.
//
// Replaces the reference's vendored Marlin path (src/kernels/quantization/marlin/*:
// marlin::gptq_gemm gptq_gemm.cu:585-710, marlin::gptq_repack gptq_repack.cu:252,
// marlin::awq_repack awq_repack.cu:191, permute_cols_kernel gptq_gemm.cu:69-118) with a layout
// and a kernel designed for the CDNA4 matrix core (v_mfma_f32_32x32x16_{bf16,f16}, wave64):
//
//  packed weights  wq[K/64][N/32][64 lanes][4] u32 (kt-major): lane l, word j = the 8 weights
//      n = 32*nt + (l & 31),  k = 64*kt + 16*j + 8*(l >> 5) + e,  e = 0..7
//    i.e. exactly the B-operand fragment of one 32x32x16 MFMA, so a wave's 16-B/lane load is one
//    contiguous KiB that feeds 4 MFMA k-steps with NO shuffle and NO LDS round trip.  kt-major
//    order: at one k position the column tiles of all concurrently running waves are adjacent in
//    memory, so the chip reads one dense N/32-KiB stripe at a time (an nt-major order makes every
//    wave stream at a power-of-two stride from its neighbours: measured HBM-channel pile-up,
//    ~2.2 TB/s ceiling).  Nibbles are
//    pair-interleaved (bit 4i = e 2i, bit 16+4i = e 2i+1) so `(w >> 4i) & 0x000F000F | magic`
//    yields a packed 16-bit pair directly (v_and_or_b32).
//  scale/zero table sz[G][N] u32 = { scale : T, magic+zero : T }  (magic = 128 bf16 / 1024 fp16;
//    the sum is exact in T), one 4-byte load per (group, column).
//  dequant: w = (q - z) * s, bit-identical to "dequantise in T then multiply" (reference
//    marlin/numeric_conversion.h:19-62,121-166,232-240: magic-number int4 -> T, sub zp, scale):
//      fp16: v_pk_add_f16 (exact) + v_pk_mul_f16 (RN);  bf16 (no packed bf16 VALU on gfx950):
//      fp32 fma(128+q, s, -(128+z)s) is exact, then v_cvt_pk_bf16_f32 (RN).
//  GEMM: C[M,N] = A[M,K] . W[K,N]; activations are the MFMA A operand (rows = tokens), staged
//    per 128-deep K chunk through XOR-swizzled LDS (conflict-free ds_read_b128); weights go
//    HBM -> registers -> dequant -> MFMA B operand; fp32 accumulate; optional split-K with fp32
//    partials + reduce (bias added after the reduction, as qlinear_awq_marlin_impl.cpp:357-363).
//
// This file holds the prepack / dequant / act-order permute kernels, the two split-K reduce kernels and the
// one entry point, slm_w4a16_gemm.  Its plan (w4_plan.hip: one planner per kernel, tried in precedence
// order; slm_w4a16_gemm_plan shows the result) picks among eight launch forms:
//    GEMV     M == 1 (M <= 4 forced)          w4_gemv.hip     dot2 GEMV, K split inside the workgroup
//    KS       M <= 32; 33 <= M <= 64 alone    w4_ks.hip       K-sliced weight stream, one / two row tiles
//    SMALL    M <= 32 where KS steps aside    w4_small.hip    lean weight stream (MFMA, post-scaled)
//    GENERAL  everything else                 w4_general.hip  32 / 64 / 128-row tiles
//    M128     65 <= M <= 128, deep wide K x N w4_m128.hip     all rows in one workgroup
//    WS       M > 128, >= 112 tiles of 256x128 w4_ws.hip      producer / consumer waves, LDS-DMA activations
//    XL       prefill-sized M x N             w4_xl.hip       symmetric 256 x 256 tiles
//    XL_SK    ... part-filled rounds of them  w4_xl.hip       the same tiles, stream-K
// (DESIGN.md 3.3 has the measurements behind each boundary.)
#include "w4_plan.h"
#include "tuning.h"

namespace slm {

__device__ __forceinline__ int awq_pos(int col_in_word) {  // [0,2,4,6,1,3,5,7] interleave
  return (col_in_word >> 1) + 4 * (col_in_word & 1);
}

// SLM_W4_PAIRED: the checkpoint tensor is a merged [gate | up] column-parallel weight
// (layers/linear/multi_parallel_linear.cpp:14-41 concatenates the two along N); its packed form
// interleaves the halves by 32-column tile -- packed tile 2j = gate tile j, packed tile 2j+1 = up
// tile j -- so the wave (pair) that owns gate columns also owns the matching up columns and can
// apply SiLU*mul in the GEMM epilogue (SLM_W4_SILU_MUL).
__device__ __forceinline__ int64_t paired_src_col(int format, int64_t n_packed, int64_t N) {
  if (!(format & SLM_W4_PAIRED)) return n_packed;
  return (n_packed >> 6) * 32 + (n_packed & 31) + ((n_packed & 32) ? N / 2 : 0);
}

// ------------------------------------------------------------------------------------------
// prepack: checkpoint formats -> wq / sz   (bit-exact integer work)
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) w4_prepack_weight_kernel(
    int format, const uint32_t* __restrict__ qweight, const int* __restrict__ perm, int64_t K,
    int64_t N, uint32_t* __restrict__ wq) {
  const int64_t widx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (widx >= N * K / 8) return;
  const int j = (int)(widx & 3);
  const int lane = (int)((widx >> 2) & 63);
  const int64_t tile = widx >> 8;
  const int64_t nt = tile % (N / 32), kt = tile / (N / 32);  // kt-major: see layout note
  const int64_t n = paired_src_col(format, nt * 32 + (lane & 31), N);
  const int64_t kb = kt * 64 + j * 16 + (lane >> 5) * 8;
  uint32_t out = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t k = perm ? (int64_t)perm[kb + e] : kb + e;
    uint32_t q;
    if (k < 0)  // padding row of an uneven act-order shard: its activation column is gathered as 0
      q = 0u;
    else if ((format & SLM_W4_FORMAT_MASK) == SLM_W4_GPTQ)
      q = (qweight[(k / 8) * N + n] >> (4 * (k % 8))) & 0xFu;
    else
      q = (qweight[k * (N / 8) + n / 8] >> (4 * awq_pos((int)(n % 8)))) & 0xFu;
    const int pos = (e >> 1) + 4 * (e & 1);
    out |= q << (4 * pos);
  }
  wq[widx] = out;
}

__global__ void __launch_bounds__(256) w4_prepack_sz_kernel(
    int format, const uint32_t* __restrict__ qzeros, const uint16_t* __restrict__ scales, int64_t G,
    int64_t N, int dtype, uint32_t* __restrict__ sz) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G * N) return;
  const int64_t g = idx / N, n = paired_src_col(format, idx % N, N);
  uint32_t z = 8u;  // no zero-point tensor: symmetric quantisation, zero = 2^(bits-1) (Marlin has_zp = false)
  if (qzeros) {
    const uint32_t zw = qzeros[g * (N / 8) + n / 8];
    if ((format & SLM_W4_FORMAT_MASK) == SLM_W4_GPTQ)
      z = ((zw >> (4 * (n % 8))) & 0xFu) + 1u;  // qlinear_impl.cpp:45 (zeros.add_(1))
    else
      z = (zw >> (4 * awq_pos((int)(n % 8)))) & 0xFu;
  }
  const uint32_t zm = (dtype == SLM_BF16 ? 0x4300u : 0x6400u) + z;  // 128 + z  /  1024 + z
  sz[idx] = (uint32_t)scales[g * N + n] | (zm << 16);
}

// debug / parity: dense W[K, N] in T from the packed form (uses W4Dq = the GEMM's dequant)
template <typename T>
__global__ void __launch_bounds__(256) w4_dequant_kernel(const uint32_t* __restrict__ wq,
                                                         const uint32_t* __restrict__ sz, int64_t K,
                                                         int64_t N, int64_t gs,
                                                         uint16_t* __restrict__ w_out) {
  const int64_t widx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (widx >= N * K / 8) return;
  const int j = (int)(widx & 3);
  const int lane = (int)((widx >> 2) & 63);
  const int64_t tile = widx >> 8;
  const int64_t nt = tile % (N / 32), kt = tile / (N / 32);  // kt-major: see layout note
  const int64_t n = nt * 32 + (lane & 31);
  const int64_t kb = kt * 64 + j * 16 + (lane >> 5) * 8;
  const W4Dq<T> dq(sz[(kb / gs) * N + n]);
  uint32_t o[4];
  dq.word(wq[widx], o);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    w_out[(kb + 2 * i) * N + n] = (uint16_t)(o[i] & 0xffffu);
    w_out[(kb + 2 * i + 1) * N + n] = (uint16_t)(o[i] >> 16);
  }
}

// A'[m, k] = A[m, perm[k]]  (act-order; reference permute_cols_kernel gptq_gemm.cu:69-118)
__global__ void __launch_bounds__(256) w4_permute_cols_kernel(const uint16_t* __restrict__ a,
                                                              const int* __restrict__ perm,
                                                              int64_t M, int64_t K, int64_t lda,
                                                              uint16_t* __restrict__ out) {
  const int64_t m = blockIdx.y;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K;
       k += (int64_t)gridDim.x * blockDim.x)
    out[m * K + k] = perm[k] >= 0 ? a[m * lda + perm[k]] : (uint16_t)0;  // < 0: padding column (+0.0)
}

// the plain split-K reduce is common.h's splitk_reduce_kernel.  SLM_W4_SILU_MUL with split-K: C[m, i] = T( silu(g) * u ), g / u = T( sum_s part[s][m][col] + bias )
// at the gate / up columns of output column i (packed tile pair 2j, 2j+1; N = packed width)
template <typename T>
__global__ void __launch_bounds__(256) w4_splitk_reduce_silu_kernel(
    const float* __restrict__ part, const void* __restrict__ bias, void* __restrict__ c, int64_t M,
    int64_t N, int64_t ldc, int split_k) {
  const int64_t idx4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // 4 output columns per thread
  const int64_t half = N / 2;
  if (idx4 * 4 >= M * half) return;
  const int64_t m = (idx4 * 4) / half, oc = (idx4 * 4) % half;
  const int64_t gc = (oc >> 5) * 64 + (oc & 31);
  f32x4 g = splitk_sum4(part + m * N + gc, M * N, split_k);
  f32x4 u = splitk_sum4(part + m * N + gc + 32, M * N, split_k);
  if (bias) {
    const uint16_t* bp = reinterpret_cast<const uint16_t*>(bias) + gc;
    const u32x2 bg = *reinterpret_cast<const u32x2*>(bp);
    const u32x2 bu = *reinterpret_cast<const u32x2*>(bp + 32);
    g.x += lo_f32<T>(bg.x); g.y += hi_f32<T>(bg.x); g.z += lo_f32<T>(bg.y); g.w += hi_f32<T>(bg.y);
    u.x += lo_f32<T>(bu.x); u.y += hi_f32<T>(bu.x); u.z += lo_f32<T>(bu.y); u.w += hi_f32<T>(bu.y);
  }
  u32x2 r;
  r.x = pack2<T>(silu_mul_acc<T>(g.x, u.x), silu_mul_acc<T>(g.y, u.y));
  r.y = pack2<T>(silu_mul_acc<T>(g.z, u.z), silu_mul_acc<T>(g.w, u.w));
  *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(c) + m * ldc + oc) = r;
}

}  // namespace slm

using namespace slm;

static bool w4_format_ok(int32_t format, int64_t N) {
  return w4_format_valid(format) && (!(format & SLM_W4_PAIRED) || N % 64 == 0);
}

extern "C" {

SLM_API size_t slm_w4_packed_weight_bytes(int64_t K, int64_t N) {
  if (K <= 0 || N <= 0 || K % 64 || N % 32) return 0;
  return (size_t)K * N / 2;
}

SLM_API size_t slm_w4_packed_sz_bytes(int64_t K, int64_t N, int64_t group_size) {
  if (K <= 0 || N <= 0 || group_size <= 0 || K % group_size) return 0;
  return (size_t)(K / group_size) * N * sizeof(uint32_t);
}

SLM_API int slm_w4_prepack_weights(int32_t format, const int32_t* qweight, const int32_t* perm,
                                   int64_t K, int64_t N, void* wq_out, void* stream) {
  if (!qweight || !wq_out) return SLM_ERR_INVALID_ARG;
  if (!w4_format_ok(format, N)) return SLM_ERR_UNSUPPORTED;
  if (K <= 0 || N <= 0 || K % 64 || N % 32) return SLM_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hip_clear_error();
  const int64_t words = K * N / 8;
  hipLaunchKernelGGL(w4_prepack_weight_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0,
                     st, format, reinterpret_cast<const uint32_t*>(qweight), perm, K, N,
                     reinterpret_cast<uint32_t*>(wq_out));
  return hip_check_launch();
}

SLM_API int slm_w4_prepack_sz(int32_t format, const int32_t* qzeros, const void* scales, int64_t K,
                              int64_t N, int64_t group_size, int32_t dtype, void* sz_out,
                              void* stream) {
  if (!scales || !sz_out) return SLM_ERR_INVALID_ARG;
  if (!w4_format_ok(format, N)) return SLM_ERR_UNSUPPORTED;
  if (dtype != SLM_F16 && dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  if (K <= 0 || N <= 0 || N % 32 || group_size <= 0 || K % group_size) return SLM_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hip_clear_error();
  const int64_t G = K / group_size;
  hipLaunchKernelGGL(w4_prepack_sz_kernel, dim3((unsigned)((G * N + 255) / 256)), dim3(256), 0, st,
                     format, reinterpret_cast<const uint32_t*>(qzeros),
                     reinterpret_cast<const uint16_t*>(scales), G, N, dtype,
                     reinterpret_cast<uint32_t*>(sz_out));
  return hip_check_launch();
}

SLM_API int slm_w4_prepack(int32_t format, const int32_t* qweight, const int32_t* qzeros,
                           const void* scales, const int32_t* perm, int64_t K, int64_t N,
                           int64_t group_size, int32_t dtype, void* wq_out, void* sz_out,
                           void* stream) {
  if (!qweight || !qzeros || !scales || !wq_out || !sz_out) return SLM_ERR_INVALID_ARG;
  if (K <= 0 || N <= 0 || K % 64 || N % 32 || group_size <= 0 || K % group_size)
    return SLM_ERR_UNSUPPORTED;
  if (dtype != SLM_F16 && dtype != SLM_BF16) return SLM_ERR_UNSUPPORTED;
  const int rc = slm_w4_prepack_weights(format, qweight, perm, K, N, wq_out, stream);
  if (rc != SLM_OK) return rc;
  return slm_w4_prepack_sz(format, qzeros, scales, K, N, group_size, dtype, sz_out, stream);
}

SLM_API int slm_w4_dequant(const void* wq, const void* sz, int64_t K, int64_t N,
                           int64_t group_size, int32_t dtype, void* w_out, void* stream) {
  if (!wq || !sz || !w_out) return SLM_ERR_INVALID_ARG;
  if (K <= 0 || N <= 0 || K % 64 || N % 32 || group_size < 16 || K % group_size)
    return SLM_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hip_clear_error();
  const int64_t words = K * N / 8;
  const dim3 grid((unsigned)((words + 255) / 256)), blk(256);
  if (dtype == SLM_BF16)
    hipLaunchKernelGGL(w4_dequant_kernel<bf16_tag>, grid, blk, 0, st, (const uint32_t*)wq,
                       (const uint32_t*)sz, K, N, group_size, (uint16_t*)w_out);
  else if (dtype == SLM_F16)
    hipLaunchKernelGGL(w4_dequant_kernel<f16_tag>, grid, blk, 0, st, (const uint32_t*)wq,
                       (const uint32_t*)sz, K, N, group_size, (uint16_t*)w_out);
  else
    return SLM_ERR_UNSUPPORTED;
  return hip_check_launch();
}

}  // extern "C"

// np != NULL: the activations are produced by the GEMV's norm prologue (slm_w4a16_gemv_norm)
static int gemm_impl(const slm_w4_gemm_args* a, const slm_w4_norm_prologue* np, void* stream) {
  GemmPlan pl;
  int rc = plan_gemm(a, &pl);
  if (rc != SLM_OK) return rc;
  if (a->M == 0) return SLM_OK;
  if (np && (pl.kernel != W4Kernel::GEMV || a->perm || !gemv_supported(a->M, a->K, a->group_size, true)))
    return SLM_ERR_UNSUPPORTED;
  if ((!np && !a->a) || !a->wq || !a->sz || !a->c) return SLM_ERR_INVALID_ARG;
  const bool silu = (a->flags & SLM_W4_SILU_MUL) != 0;
  if (np) {
    // exactly one activation source; the residual is double-buffered: every workgroup recomputes
    // x + residual_in while workgroup 0 stores residual_out, so the two must not share memory
    if (!np->weight || (np->x != nullptr) == (np->partials != nullptr) ||
        (np->partials && np->n_splits < 1) || (np->residual_in && !np->residual_out))
      return SLM_ERR_INVALID_ARG;
    const size_t row_bytes = (size_t)a->M * a->K * 2;
    auto overlaps = [&](const void* w, const void* r) {
      const char* wp = reinterpret_cast<const char*>(w);
      const char* rp = reinterpret_cast<const char*>(r);
      return w && r && wp < rp + row_bytes && rp < wp + row_bytes;
    };
    if (overlaps(np->residual_out, np->residual_in) || overlaps(np->residual_out, np->x) ||
        overlaps(np->normed_out, np->residual_in) || overlaps(np->normed_out, np->x) ||
        overlaps(np->normed_out, np->residual_out))
      return SLM_ERR_INVALID_ARG;
    if (!aligned16(np->x) || !aligned16(np->partials) || !aligned16(np->residual_in) ||
        !aligned16(np->residual_out) || !aligned16(np->weight) || !aligned16(np->normed_out))
      return SLM_ERR_ALIGNMENT;
  }
  // with perm the packed K may exceed the source width (padded act-order shards): perm[k] < lda is
  // the caller's contract then
  if ((!np && (!aligned16(a->a) || a->lda % 8 || (!a->perm && a->lda < a->K))) || !aligned16(a->wq) ||
      a->ldc < (silu ? a->N / 2 : a->N))
    return SLM_ERR_ALIGNMENT;
  if ((pl.part_bytes + pl.aperm_bytes) > 0 &&
      (!a->workspace || a->workspace_bytes < pl.part_bytes + pl.aperm_bytes))
    return SLM_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hip_clear_error();

  GemmKParams kp;
  kp.a = a->a; kp.lda = a->lda;
  kp.norm_weight = nullptr;
  if (np) {
    kp.a = nullptr; kp.lda = a->K;
    kp.norm_x = np->x; kp.norm_part = np->partials; kp.norm_splits = np->n_splits;
    kp.norm_eps = np->eps; kp.norm_res_in = np->residual_in; kp.norm_res_out = np->residual_out;
    kp.norm_weight = np->weight; kp.norm_out = np->normed_out;
  }
  if (a->perm) {  // act-order: gather the activation columns once (gptq_gemm.cu:69-118)
    uint16_t* ap = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(a->workspace) + pl.part_bytes);
    const unsigned gx = (unsigned)((a->K + 255) / 256);
    hipLaunchKernelGGL(w4_permute_cols_kernel, dim3(gx > 64 ? 64 : gx, (unsigned)a->M), dim3(256), 0,
                       st, reinterpret_cast<const uint16_t*>(a->a), a->perm, a->M, a->K, a->lda, ap);
    rc = hip_check_launch();
    if (rc != SLM_OK) return rc;
    kp.a = ap; kp.lda = a->K;
  }
  kp.wq = reinterpret_cast<const uint32_t*>(a->wq);
  kp.sz = reinterpret_cast<const uint32_t*>(a->sz);
  kp.bias = a->bias; kp.c = a->c;
  kp.part = pl.split_k > 1 ? reinterpret_cast<float*>(a->workspace) : nullptr;
  kp.M = a->M; kp.K = a->K; kp.N = a->N; kp.ldc = a->ldc;
  // per-channel scales (group_size == K, not necessarily a power of two): every k maps to group 0
  kp.gs_shift = (a->group_size == a->K) ? 30 : ilog2(a->group_size);
  kp.n_chunks = (int)(a->K / W4_KC);
  kp.split_k = pl.split_k; kp.chunks_per_split = pl.chunks_per_split;
  kp.n_mblocks = pl.n_mblocks; kp.n_nblocks = pl.n_nblocks;
  kp.silu = silu ? 1 : 0;
  kp.ks_tpw = pl.ks.tpw;
  kp.ks_groups = (int)(a->K / a->group_size);
  kp.sk_per = pl.xl_sk.sk_per; kp.sk_sync = nullptr; kp.sk_part = nullptr;
  switch (pl.kernel) {
    case W4Kernel::GEMV: launch_gemv(kp, a->dtype, pl, st); break;
    case W4Kernel::KS: launch_gemm_ks(kp, a->dtype, pl, st); break;
    case W4Kernel::SMALL: launch_gemm_small(kp, a->dtype, pl, st); break;
    case W4Kernel::GENERAL: launch_gemm_general(kp, a->dtype, pl, st); break;
    case W4Kernel::M128: launch_gemm_m128(kp, a->dtype, pl, st); break;
    case W4Kernel::WS: launch_gemm_ws(kp, a->dtype, pl, st); break;
    case W4Kernel::XL: launch_gemm_xl(kp, a->dtype, pl, st); break;
    case W4Kernel::XL_SK:
      kp.sk_part = reinterpret_cast<float*>(a->workspace);
      kp.sk_sync = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(a->workspace) + W4_XL_SK_WGS * W4_XL_SK_SLOT_BYTES);
      // the ticket and the flags start at zero on every call (a memset node under capture)
      if (hipMemsetAsync(kp.sk_sync, 0, W4_XL_SK_SYNC_BYTES, st) != hipSuccess) return hip_check_launch();
      launch_gemm_xl_sk(kp, a->dtype, pl, st);
      break;
  }
  rc = hip_check_launch();
  if (rc != SLM_OK) return rc;
  if (pl.split_k > 1 && !((a->flags & SLM_W4_DEFER_REDUCE) && !a->bias)) {
    dispatch_dtype(a->dtype, [&](auto t) {
      using T = decltype(t);
      if (silu) {
        const int64_t n4 = a->M * (a->N / 2) / 4;
        hipLaunchKernelGGL(w4_splitk_reduce_silu_kernel<T>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st,
                           kp.part, a->bias, a->c, a->M, a->N, a->ldc, pl.split_k);
      } else {
        launch_splitk_reduce<T>(kp.part, a->bias, a->c, a->M, a->N, a->ldc, pl.split_k, st);
      }
    });
    rc = hip_check_launch();
  }
  return rc;
}

extern "C" {

SLM_API int slm_w4a16_gemm(const slm_w4_gemm_args* a, void* stream) {
  return gemm_impl(a, nullptr, stream);
}

SLM_API int slm_w4a16_gemv_norm(const slm_w4_gemm_args* a, const slm_w4_norm_prologue* np,
                                void* stream) {
  if (!a || !np) return SLM_ERR_INVALID_ARG;
  return gemm_impl(a, np, stream);
}

}  // extern "C"
