/*
 * slm_hip.h -- C ABI of libslm_hip.so: the MI355X (gfx950 / CDNA4) kernel library
 * behind ScaleLLM's decode hot path.
 *
 * Drop-in boundary: every entry point below replaces one C++ kernel-level
 * symbol of the reference (vectorch-ai/ScaleLLM, paths relative to the
 * reference root).  The reference passes torch::Tensor; a thin libtorch shim
 * (scalellm_amd/csrc/shim/) adapts tensor -> (pointer,
 * strides, sizes) and calls these functions, so the reference src/layers tree compiles
 * unchanged.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes only; no torch / C++ types;
 *   - device pointers unless stated "host";
 *   - asynchronous on `stream` (a hipStream_t passed as void*); never
 *     synchronises, never allocates, never reads device memory on the host --
 *     therefore safe under hipGraph stream capture (the only exceptions are the
 *     init-time slm_shm_* / slm_ar_read_error helpers of section 6, marked there)
 *     (reference: src/engine/model_runner.cpp:141-178);
 *   - returns 0 (SLM_OK) or a negative slm_status; never aborts;
 *   - thread-safe per stream (one Worker thread per GPU in the reference:
 *     src/engine/worker.cpp:202-213).
 */
#ifndef SLM_HIP_H_
#define SLM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLM_API __attribute__((visibility("default")))

typedef enum slm_status {
  SLM_OK = 0,
  SLM_ERR_INVALID_ARG = -1,   /* null pointer, bad size, non power-of-two block_size ... */
  SLM_ERR_UNSUPPORTED = -2,   /* dtype / head_dim / bits / group not supported */
  SLM_ERR_WORKSPACE = -3,     /* workspace missing or too small */
  SLM_ERR_LAUNCH = -4,        /* hipLaunchKernel reported an error */
  SLM_ERR_ALIGNMENT = -5      /* pointer or stride not 16-byte aligned */
} slm_status;

typedef enum slm_dtype {
  SLM_F16 = 0,  /* IEEE half   (torch::kHalf)     */
  SLM_BF16 = 1, /* bfloat16    (torch::kBFloat16) */
  SLM_F32 = 2   /* IEEE float  (torch::kFloat32): the logits of sections 8 / 9, the rows of section 14 */
} slm_dtype;

SLM_API const char* slm_status_string(int status);
SLM_API const char* slm_version(void);
/* hipGetErrorString of the last launch status seen by this thread (detail for SLM_ERR_LAUNCH). */
SLM_API const char* slm_last_hip_error(void);

/* ========================================================================== */
/* 0. Launch-shape overrides (sweeps, tests that force one kernel).           */
/*    The library never reads the environment per call: the SLM_* variables   */
/*    (SLM_ATTN_NW, SLM_ATTN_SPLITS, SLM_W4_MT, SLM_W4_SPLITK ... -- the full */
/*    list is scalellm_amd/csrc/tuning.h) are parsed ONCE, at first use, and   */
/*    only these calls change a knob afterwards.  Process-wide; not meant to  */
/*    be flipped while other threads launch.  name = the variable's name.     */
/*    slm_tuning_clear(NULL) clears every knob (environment values included). */
/* ========================================================================== */
SLM_API int slm_tuning_set(const char* name, int32_t value);
SLM_API int slm_tuning_clear(const char* name);
SLM_API int slm_tuning_get(const char* name, int32_t* value, int32_t* is_set);

/* ========================================================================== */
/* 1. Paged-KV varlen attention (prefill / chunked prefill / decode / verify) */
/*    replaces  llm::paged_kv_varlen_mha                                      */
/*              src/kernels/attention/attn_api.h:12-27 (impl attn_api.cpp:14) */
/*    caller    ScaleAttnHandler::batch_decode                                */
/*              src/layers/attention/scale_attn_handler.cpp:44-68             */
/*    params    mirror MHAPagedKVParams, src/kernels/attention/mha_params.h   */
/*              :11-117 (strides in ELEMENTS; last dim contiguous).           */
/*    Block table = flattened first-slot ids + CSR offsets                    */
/*    (src/engine/batch.cpp:206-209, src/models/parameters.h:50-55);          */
/*    slot(kv_idx) = block_table[block_cu_lens[b] + (kv_idx >> log2(bs))]     */
/*                   + (kv_idx & (bs-1))   (kernel/sm80_kernel_mha.cuh:146).  */
/* ========================================================================== */
typedef struct slm_attn_args {
  void* out;                /* [n_tokens, n_heads, head_dim]                  */
  const void* query;        /* [n_tokens, n_heads, head_dim]                  */
  const void* key_cache;    /* [n_slots, n_kv_heads, head_dim]                */
  const void* value_cache;  /* [n_slots, n_kv_heads, head_dim]                */
  int64_t o_stride[2];      /* {token stride, head stride} in elements        */
  int64_t q_stride[2];
  int64_t k_stride[2];      /* {slot stride, head stride}                     */
  int64_t v_stride[2];
  const int32_t* q_cu_lens;      /* [batch+1]                                 */
  const int32_t* kv_cu_lens;     /* [batch+1]                                 */
  const int32_t* block_table;    /* [sum_b ceil(kv_len_b / block_size)]       */
  const int32_t* block_cu_lens;  /* [batch+1]                                 */
  const float* alibi_slopes;     /* [n_heads] or NULL                         */
  int32_t dtype;            /* slm_dtype of out/query/caches                  */
  int32_t batch_size;
  int32_t n_tokens;         /* = query.size(0) = q_cu_lens[batch].  Only a pure-decode batch (max_q_len <= 1)
                             * may carry MORE rows than q_cu_lens[batch]: the graph padding of batch.cpp:219-244,
                             * left untouched.  (With max_q_len > 1 the plan relies on the equality: when
                             * n_tokens == batch_size * max_q_len every sequence has max_q_len tokens and only
                             * that row class is launched.) */
  int32_t n_heads;
  int32_t n_kv_heads;
  int32_t head_dim;         /* multiple of 8, <= 256                          */
  int32_t block_size;       /* power of two (mha_params.h:71-74)              */
  int32_t max_q_len;        /* scheduling hint, as in the reference           */
  int32_t max_kv_len;       /* scheduling hint (unused by the reference): sizes the KV splits /
                             * the balanced decode partition.  Results are correct for ANY value:
                             * a sequence longer than the hint is streamed by one workgroup
                             * (slower, never wrong or out of bounds)                          */
  float sm_scale;
  float logits_soft_cap;    /* 0 = off                                        */
  int32_t sliding_window;   /* -1 = off                                       */
  void* workspace;          /* split-KV scratch, may be NULL if bytes == 0    */
  size_t workspace_bytes;
  int32_t num_splits;       /* 0 = auto (heuristic); >0 forces the split count */
  int32_t total_kv_len;     /* scheduling hint, 0 = unknown: kv_cu_lens[batch] if the host has it
                             * (Batch::prepare_model_input builds cu_seq_lens on the host, batch.cpp:137).
                             * total_kv_len == batch_size * max_kv_len tells the plan that every sequence
                             * has max_kv_len tokens: a pure-decode call that needs no KV split then skips
                             * the balanced partition and with it the combine launch that would find
                             * nothing to merge.  Like max_kv_len it only shapes the launch: results are
                             * correct whatever the value (a wrong "uniform" claim costs balance, not bits) */
  int32_t phase;            /* 0 = the whole call (default).  A call that splits the KV range runs as stream
                             * kernel(s) + a combine pass; a host that overlaps calls on two streams (the two
                             * decode lanes) may issue the halves separately: 1 = everything BUT
                             * the combine pass, 2 = the combine pass only (a no-op when the plan needs none).
                             * Same arguments for both; phase 1 then phase 2 on one stream == phase 0. */
  int32_t n_slots;          /* slots the two caches hold (key_cache.size(0)), 0 = unknown.  The LDS-DMA prefill forms of
                             * the tile kernel address the caches through a buffer descriptor, and the buffer unit
                             * keeps slot * stride to 32 bits (attn_tile.hip): they are taken only when n_slots is
                             * known and n_slots * slot stride <= 4 GiB for both caches; otherwise the rows run
                             * on the register-staged form (64-bit addresses), whatever SLM_ATTN_TILE_PF says.
                             * It only chooses between forms that compute the same bits. */
} slm_attn_args;

/* Scratch needed for `a` (depends only on host-side sizes; AttentionHandler::
 * get_estimate_workspace_size / set_workspace, src/layers/attention/handler.h
 * :40-47 is the natural home).  Pass num_splits to query a forced split count.*/
SLM_API size_t slm_paged_kv_varlen_mha_workspace_bytes(const slm_attn_args* a);
/* Split count the heuristic would pick for `a` (host-side sizes only).        */
SLM_API int32_t slm_paged_kv_varlen_mha_auto_splits(const slm_attn_args* a);
/* which kernel the plan gives the q_len = 1 (decode) rows of this call: 0 = attn_token_kernel (HBM
 * stream, dot2), 1 = attn_tile_kernel (MFMA tile form: wide GQA groups), -1 = invalid arguments.
 * A pure function of the argument block and the tuning table (what a bench labels its roofline with). */
SLM_API int32_t slm_paged_kv_varlen_mha_decode_kernel(const slm_attn_args* a);
/* whether the call may take the LDS-DMA prefill forms of the tile kernel: 1 = n_slots is given and both caches end
 * within 4 GiB of their pointers, 0 = not (n_slots 0 or larger caches: register-staged forms), -1 = invalid
 * arguments.  Host-side; what a test or a bench asserts so that a forgotten n_slots does not pass as a slower prefill. */
SLM_API int32_t slm_paged_kv_varlen_mha_kv_near(const slm_attn_args* a);
SLM_API int slm_paged_kv_varlen_mha(const slm_attn_args* a, void* stream);

/* ========================================================================== */
/* 2. KV-cache append                                                         */
/*    replaces  llm::kernel::set_kv_cache                                     */
/*              src/kernels/kv_cache_kernels.h:6-11 (.cu:9-78)                */
/*    caller    KVCache::set_kv_cache_cuda  src/memory/kv_cache.cpp:53-57     */
/*    cache[slot_ids[t], h, d] = kv[t, h, d] for K and V (bit-exact copy).    */
/* ========================================================================== */
SLM_API int slm_set_kv_cache(const int32_t* slot_ids,  /* [n_tokens]           */
                             const void* keys,         /* [n_tokens, n_kv_heads, head_dim] */
                             const void* values,
                             int64_t k_token_stride,   /* elements             */
                             int64_t v_token_stride,
                             void* key_cache,          /* [n_slots, n_kv_heads, head_dim] contiguous */
                             void* value_cache,
                             int64_t n_tokens, int32_t n_kv_heads, int32_t head_dim,
                             int32_t dtype, void* stream);

/* ========================================================================== */
/* 3. int4 weight prepack (checkpoint format -> MFMA-native layout)           */
/*    replaces  marlin::gptq_repack / marlin::awq_repack                      */
/*              src/kernels/quantization/marlin.h:27-35                       */
/*              (gptq_repack.cu:252, awq_repack.cu:191) and the host-side     */
/*              scale / zero-point permutations of                            */
/*              qlinear_awq_marlin_impl.cpp:34-125,                           */
/*              qlinear_gptq_marlin_impl.cpp:41-71.                           */
/*    Inputs are the stable on-disk formats:                                  */
/*      GPTQ: qweight [K/8, N] int32 (nibble k%8 at bit 4*(k%8)),             */
/*            qzeros  [G, N/8] int32 (plain order, zero = stored + 1),        */
/*            scales  [G, N] T, optional g_idx [K] (act-order);               */
/*      AWQ : qweight [K, N/8] int32, qzeros [G, N/8] int32, both with the    */
/*            [0,2,4,6,1,3,5,7] nibble interleave, zero = stored;             */
/*            scales  [G, N] T.                                               */
/*    Output layout (owned by this library):                   */
/*      wq  [K/64][N/32][64 lanes][4] uint32  -- lane l, word j holds the 8   */
/*           nibbles n = 32*nt + (l&31), k = 64*kt + 16*j + 8*(l>>5) + p'     */
/*           in a pair-interleaved nibble order (MFMA 32x32x16 B-fragment);   */
/*      sz  [G][N] {scale, magic + zero} as 2 x T (magic = 128 for bf16,      */
/*           1024 for fp16: the sum is exact in T; fused scale/zero table);   */
/*      perm[K] int32 (act-order only): row k' of wq = checkpoint row perm[k']*/
/*           perm[k'] < 0 marks a PADDING row (weights 0, activation column   */
/*           gathered as +0.0): a row-parallel act-order shard               */
/*           (qlinear_gptq_marlin_impl.cpp:236-243: sharded g_idx, full       */
/*           scales) holds an uneven number of rows of every group, so the    */
/*           host pads each group's sorted rows to a multiple of 32 and packs */
/*           with K = the padded row count, group_size = 32 and one scale row */
/*           per 32-row block (tools: kernels.gptq_repack / slm::W4Linear).   */
/* ========================================================================== */
typedef enum slm_w4_format {
  SLM_W4_GPTQ = 0,
  SLM_W4_AWQ = 1,
  SLM_W8_GPTQ = 2, /* 8-bit checkpoints: slm_w8_prepack_* only (section 3b) */
  SLM_W8_AWQ = 3
} slm_w4_format;
#define SLM_W4_FORMAT_MASK 0xF
/* OR into `format`: the checkpoint tensors are a merged [gate | up] column-parallel weight (the
 * reference builds it by concatenating gate_proj and up_proj along N,
 * layers/linear/multi_parallel_linear.cpp:14-41; N = 2 * intermediate, N % 64 == 0).  The packed
 * form then interleaves the two halves by 32-column tile -- packed tile 2j = columns
 * [32j, 32j+32) of gate, packed tile 2j+1 = the same columns of up -- which is what lets
 * slm_w4a16_gemm apply SiLU*mul in its epilogue (SLM_W4_SILU_MUL).  Without that flag a GEMM on
 * paired weights returns the columns in the packed (interleaved) order. */
#define SLM_W4_PAIRED 0x10

SLM_API size_t slm_w4_packed_weight_bytes(int64_t K, int64_t N);
SLM_API size_t slm_w4_packed_sz_bytes(int64_t K, int64_t N, int64_t group_size);

SLM_API int slm_w4_prepack(int32_t format,            /* slm_w4_format          */
                           const int32_t* qweight, const int32_t* qzeros,
                           const void* scales,        /* [G, N] T               */
                           const int32_t* perm,       /* [K] sorted-row -> ckpt-row, or NULL */
                           int64_t K, int64_t N, int64_t group_size, int32_t dtype,
                           void* wq_out, void* sz_out, void* stream);
/* The two halves of slm_w4_prepack, for callers that hold the weights and the scale / zero-point
 * tensors at different times -- marlin::gptq_repack / awq_repack take q_weight alone
 * (marlin.h:27-35) and marlin::gptq_gemm takes scales / zeros per call (marlin.h:17-25):
 *   weights: qweight (+ perm) -> wq_out  [K*N/8 uint32, this library's layout];
 *   sz     : scales (+ qzeros) -> sz_out [G*N uint32].  qzeros == NULL means symmetric
 *            quantisation, zero = 8 (what Marlin's has_zp = false means for 4 bits). */
SLM_API int slm_w4_prepack_weights(int32_t format, const int32_t* qweight, const int32_t* perm,
                                   int64_t K, int64_t N, void* wq_out, void* stream);
SLM_API int slm_w4_prepack_sz(int32_t format, const int32_t* qzeros /* or NULL */, const void* scales,
                              int64_t K, int64_t N, int64_t group_size, int32_t dtype, void* sz_out,
                              void* stream);

/* ========================================================================== */
/* 3b. 8-bit weights (num_bits = 8 of marlin::gptq_gemm / gptq_repack /        */
/*     awq_repack, marlin.h:17-37; bits = 8 of the quantised linears,          */
/*     qlinear_awq_marlin_impl.cpp:25-26; CPU semantics construct_weights,     */
/*     qlinear_impl.cpp:21-100) as TWO int4 planes of the int4 GEMM:           */
/*       s (q - z) = (16 s)(hi - zh) + s (lo - zl),  q = 16 hi + lo            */
/*     The packed weight has 2K rows -- [0, K) high nibbles (scale 16 s,       */
/*     zero z >> 4), [K, 2K) low nibbles (scale s, zero z & 15) -- and the     */
/*     GEMM reads the activations twice through its column gather:            */
/*       slm_w4_gemm_args { K = 2K, lda = the real row stride of A,            */
/*                          perm = perm2 (written by slm_w8_prepack_weights),  */
/*                          group_size = slm_w8_packed_group_size(K, g) }      */
/*     Exact in exact arithmetic; same HBM bytes as a native 8-bit kernel,     */
/*     twice the MFMA work of an int4 GEMM (csrc/w8_planes.hip).               */
/*     Checkpoint layouts: GPTQ qweight [K/4, N] (byte k%4), qzeros [G, N/4]   */
/*     (byte n%4, zero = stored + 1), AWQ qweight [K, N/4] / qzeros [G, N/4]   */
/*     with the byte order [0,2,1,3] (tests/kernels/quant_utils.py:182-184).   */
/*     Sizes: slm_w4_packed_weight_bytes(2K, N),                               */
/*            slm_w4_packed_sz_bytes(2K, N, packed group size), perm2 [2K].    */
/* ========================================================================== */
SLM_API int64_t slm_w8_packed_rows(int64_t K);
SLM_API int64_t slm_w8_packed_group_size(int64_t K, int64_t group_size); /* 0 = unsupported */
SLM_API int slm_w8_prepack_weights(int32_t format, /* SLM_W8_* (| SLM_W4_PAIRED) */
                                   const int32_t* qweight,
                                   const int32_t* perm, /* [K] act-order sorted-row -> ckpt-row, or NULL */
                                   int64_t K, int64_t N, void* wq_out, int32_t* perm2_out /* [2K] */,
                                   void* stream);
SLM_API int slm_w8_prepack_sz(int32_t format, const int32_t* qzeros /* or NULL: symmetric, zero 128 */,
                              const void* scales /* [K / group_size, N] T */, int64_t K, int64_t N,
                              int64_t group_size, int32_t dtype, void* sz_out, void* stream);

/* ========================================================================== */
/* 4. int4-weight x fp16/bf16-activation GEMM  C[M,N] = A[M,K] . dequant(W)   */
/*    replaces  marlin::gptq_gemm  src/kernels/quantization/marlin.h:17-25    */
/*              (gptq_gemm.cu:585-710) incl. permute_cols_kernel              */
/*              (gptq_gemm.cu:69-118) for act-order.                          */
/*    callers   {Column,Row}ParallelQLinear{AWQ,GPTQ}MarlinImpl::forward      */
/*              qlinear_awq_marlin_impl.cpp:238,344;                          */
/*              qlinear_gptq_marlin_impl.cpp:188,310.                         */
/*    w = scale * (q - zero); fp32 accumulate; output rounded RN to T.        */
/* ========================================================================== */
typedef struct slm_w4_gemm_args {
  const void* a;        /* [M, K] T, row stride lda (elements)                */
  const void* wq;       /* packed by slm_w4_prepack                           */
  const void* sz;       /* packed scale/zero table                            */
  const int32_t* perm;  /* [K] act-order column gather for A (entries < lda; < 0 = zero column), or NULL */
  const void* bias;     /* [N] T or NULL (added after accumulation)           */
  void* c;              /* [M, N] T, row stride ldc                           */
  int64_t M, K, N;      /* K = packed rows; with perm, A may be narrower (padded act-order shard) */
  int64_t lda, ldc;
  int64_t group_size;   /* K for per-channel (-1 in the checkpoint)           */
  int32_t dtype;
  int32_t flags;        /* SLM_W4_* bits, 0 = none                            */
  void* workspace;      /* split-K partials + act-order A copy                */
  size_t workspace_bytes;
} slm_w4_gemm_args;

/* flags: leave a split-K GEMM's fp32 partial sums [splits][M][N] at the START of `workspace`
 * instead of reducing them into c (which is then NOT written): the consumer absorbs the sum --
 * slm_rms_norm_splitk does, removing one launch and one round trip of the activations per
 * row-parallel linear.  Ignored (normal reduce) when bias != NULL.  Whether a given call defers is
 * a pure function of the argument block: ask slm_w4a16_gemm_deferred_splits first. */
#define SLM_W4_DEFER_REDUCE 1
/* flags: wq / sz were packed with SLM_W4_PAIRED and c is [M, N/2] (ldc >= N/2):
 *   c[m, i] = T( silu(g) * u ),  g = T(acc[m, gate col i] + bias), u = T(acc[m, up col i] + bias)
 * -- bit-identical to the unfused sequence "GEMM into [M, N], then slm_silu_mul"
 * (kernel::act_and_mul, src/kernels/activation_kernels.cu:84, after the merged gate_up linear of
 * the MLP), minus one launch and the round trip of the [M, N] intermediate.  bias, if given, is in
 * packed column order.  Needs N % 64 == 0; cannot be combined with SLM_W4_DEFER_REDUCE. */
#define SLM_W4_SILU_MUL 2
/* flags: the call SHARES THE CHIP with kernels of another stream that must keep running next to it (the two
 * half-batch decode lanes of DESIGN.md 3.6: one lane's GEMMs run under the other lane's attention stream).  A
 * scheduling hint: the plan then avoids launch shapes whose workgroups cannot sit on a CU beside other waves --
 * the two-row-tile K-sliced stream for 33 <= M <= 64 (512 threads x 236 VGPRs: alone it is the faster kernel,
 * 89 vs 96 us per Llama-3-8B layer; beside an attention stream its workgroups wait for whole CUs, 14.2 -> 21.5 ms
 * at bs 128).  Results are correct either way; the SAME flag must be passed to the workspace / deferred-splits
 * queries (they describe the plan the call will take). */
#define SLM_W4_SHARES_CHIP 4

SLM_API size_t slm_w4a16_gemm_workspace_bytes(const slm_w4_gemm_args* a);
/* number of partial slabs the call will leave in the workspace (>= 2), or 0 when it writes c as usual */
SLM_API int32_t slm_w4a16_gemm_deferred_splits(const slm_w4_gemm_args* a);
/* The launch the plan gives `a`: which kernel, its grid and its kernel-specific parameters.  A pure
 * function of the argument block and the tuning table (csrc/w4_plan.hip): no HIP call, works without a
 * GPU; the two queries above are read from the same plan (workspace = part_bytes + aperm_bytes).
 * variant[] per kernel id, unused entries 0:
 *   KS      { row tiles 1 / 2, chunks of K per wave, waves per workgroup, column tiles per workgroup }
 *   GENERAL { row tiles, column tiles per wave, chunks per pass, 1 = post-scaled dequant }
 *   M128    { weight ring depth, waves per column tile, column tiles per workgroup, 1 = LDS-DMA activations }
 *   XL_SK   { 128-deep chunks of the work list per workgroup }                                        */
typedef enum slm_w4_kernel {
  SLM_W4_KERNEL_GEMV = 0,    /* w4_gemv.hip     dot2 GEMV, M <= 4                                  */
  SLM_W4_KERNEL_KS = 1,      /* w4_ks.hip       K-sliced stream, one (M <= 32) or two (M <= 64) row tiles */
  SLM_W4_KERNEL_SMALL = 2,   /* w4_small.hip    lean weight stream, M <= 32                       */
  SLM_W4_KERNEL_GENERAL = 3, /* w4_general.hip  32 / 64 / 128-row tiles                           */
  SLM_W4_KERNEL_M128 = 4,    /* w4_m128.hip     65 <= M <= 128, all rows in one workgroup         */
  SLM_W4_KERNEL_WS = 5,      /* w4_ws.hip       wave-specialised 256 x 128 tiles                  */
  SLM_W4_KERNEL_XL = 6,      /* w4_xl.hip       256 x 256 tiles                                   */
  SLM_W4_KERNEL_XL_SK = 7    /* w4_xl.hip       256 x 256 tiles, stream-K                         */
} slm_w4_kernel;
typedef struct slm_w4_plan_info {
  int32_t kernel;            /* slm_w4_kernel                                                      */
  int32_t row_tiles;         /* 32-row tiles per workgroup the kernel works on (GEMV: 0, it has no row tiles) */
  int32_t n_mblocks, n_nblocks, split_k, chunks_per_split; /* grid; chunks are 128 deep            */
  int32_t variant[4];
  uint64_t lds_bytes;        /* dynamic LDS of the launch (GEMV: without the norm prologue's row)  */
  uint64_t part_bytes, aperm_bytes; /* workspace: split-K / stream-K partials, then the act-order A copy */
} slm_w4_plan_info;
SLM_API int slm_w4a16_gemm_plan(const slm_w4_gemm_args* a, slm_w4_plan_info* out);
SLM_API int slm_w4a16_gemm(const slm_w4_gemm_args* a, void* stream);

/* The M <= 4 GEMV with the RMSNorm that feeds it computed in its prologue: at batch 1 a decoder
 * layer is launch-bound, and the norm before the qkv and gate_up projections
 * (input_layernorm_ / post_attention_layernorm_, src/models/meta/llama.h:174-176) is 8 KiB of work per token.
 *   h      = T(x) + residual_in            (fp32; x given directly or as split-K slabs)
 *   a      = rms_norm(h) * weight          (what the GEMV consumes; never leaves the chip unless
 *                                           normed_out is given)
 *   residual_out = T(h)
 * followed by the GEMM of `a` exactly as slm_w4a16_gemm does it (a->a and a->lda are ignored;
 * flags as usual).  Bit-identical to slm_rms_norm / slm_rms_norm_splitk followed by
 * slm_w4a16_gemm.  Every workgroup recomputes the norm while workgroup 0 stores residual_out /
 * normed_out, hence residual_out may not overlap residual_in or x (double-buffer the residual);
 * SLM_ERR_INVALID_ARG otherwise.  SLM_ERR_UNSUPPORTED unless slm_w4a16_gemv_norm_supported(a). */
typedef struct slm_w4_norm_prologue {
  const void* x;           /* [M, K] T contiguous, or NULL when `partials` is given         */
  const float* partials;   /* [n_splits, M, K] fp32 slabs of a deferred GEMM, or NULL       */
  int32_t n_splits;
  float eps;
  const void* residual_in; /* [M, K] T or NULL (plain rms_norm)                             */
  void* residual_out;      /* [M, K] T, required with residual_in                           */
  const void* weight;      /* [K] T                                                         */
  void* normed_out;        /* optional [M, K] T copy of the normalised activations          */
} slm_w4_norm_prologue;
/* 1 when the argument block would take the GEMV path (M <= 4, supported group size, no act-order
 * permutation, the extra fp32 row fits the LDS): a pure function of the block and the tuning table */
SLM_API int32_t slm_w4a16_gemv_norm_supported(const slm_w4_gemm_args* a);
SLM_API int slm_w4a16_gemv_norm(const slm_w4_gemm_args* a, const slm_w4_norm_prologue* np,
                                void* stream);

/* Slow dequantise-to-dense helper (debug / parity): w_out [K, N] T.          */
SLM_API int slm_w4_dequant(const void* wq, const void* sz, int64_t K, int64_t N,
                           int64_t group_size, int32_t dtype, void* w_out, void* stream);

/* ========================================================================== */
/* 5. Glue ops of one decoder layer (SURVEY 8f "next" rows f1/f2).            */
/*    replaces  kernel::apply_rotary_pos_emb  src/kernels/pos_embedding_      */
/*              kernels.cu:35-121; kernel::rms_norm / rms_norm_residual       */
/*              src/kernels/layernorm_kernels.cu:15,125;                      */
/*              kernel::act_and_mul (silu) src/kernels/activation_kernels.cu  */
/*              :84.                                                          */
/* ========================================================================== */
/* residual != NULL: x := x + residual (fp32), residual := T(x), then normalise
 * (rms_norm_residual, src/layers/normalization.h:42-52). */
SLM_API int slm_rms_norm(void* out, const void* x, const void* weight, void* residual,
                         int64_t n_tokens, int64_t dim, float eps, int32_t dtype, void* stream);
/* The same with x given as the split-K partial sums a deferred GEMM left behind
 * (SLM_W4_DEFER_REDUCE): x := T(sum_s partials[s][t][:]) in the reduce kernel's own order, so the
 * result is bit-identical to "reduce, then slm_rms_norm". */
SLM_API int slm_rms_norm_splitk(void* out, const float* partials /* [n_splits, n_tokens, dim] */,
                                int32_t n_splits, const void* weight, void* residual,
                                int64_t n_tokens, int64_t dim, float eps, int32_t dtype, void* stream);
/* LayerNorm with weight and optional bias (bias == NULL: none), fp32 statistics, one rounding:
 * out = T((x - mean) * rsqrt(var + eps) * weight + bias).  replaces kernel::layer_norm
 * (src/kernels/layernorm_kernels.cu:185-256; LayerNormImpl::forward src/layers/normalization.h:86-95)
 * for the LayerNorm model families (GPT-2: BASELINE configs[0], GPT-NeoX, Bloom, MPT).  dim % 8 == 0,
 * dim <= 16384, contiguous rows. */
SLM_API int slm_layer_norm(void* out, const void* x, const void* weight, const void* bias /* or NULL */,
                           int64_t n_tokens, int64_t dim, float eps, int32_t dtype, void* stream);
/* tanh-form GELU: kind = SLM_GELU_NEW (kernel::gelu_new, GPT-2's "gelu_new") or SLM_GELU_FAST
 * (kernel::gelu_fast), src/kernels/activation_kernels.cu:20-40,111-120.  with_mul = 0: out [T, d] =
 * act(x [T, d]);  with_mul = 1: out [T, d] = T(act(x[:, :d])) * x[:, d:], x [T, 2 d]
 * (gelu_new_with_mul / gelu_fast_with_mul, activation_kernels.cu:128-145).  d % 8 == 0. */
#define SLM_GELU_NEW 0
#define SLM_GELU_FAST 1
SLM_API int slm_gelu(void* out, const void* x, int64_t n_tokens, int64_t d, int32_t kind, int32_t with_mul,
                     int32_t dtype, void* stream);
/* Rotary embedding applied in place to q and k, fused with the KV append that always follows it
 * (src/layers/attention/attention.cpp:36-42).  cos_sin row = [cos(rot/2) | sin(rot/2)] per
 * position (the reference cache layout, pos_embedding_kernels.cu:41: [max_pos, 2, rot/2]), either
 * in the activation dtype (as RotaryEmbeddingKernel builds it, pos_embedding.cpp:195-196) or
 * fp32.  cos_sin == NULL skips the rotation (alibi models); slot_ids == NULL skips the append.
 * A token whose slot id is negative (graph padding) is rotated in place like any other, but its
 * append is skipped: neither cache is written for it.  Every other id must be a valid slot.  The
 * same holds for slm_rope_kv_append_splitk below. */
SLM_API int slm_rope_kv_append(void* q /* [T, n_heads, D] in place */, int64_t q_token_stride,
                               void* k /* [T, n_kv_heads, D] in place */, int64_t k_token_stride,
                               const void* v /* [T, n_kv_heads, D] */, int64_t v_token_stride,
                               const int32_t* positions /* [T] */,
                               const void* cos_sin /* [max_pos, rot_dim] */, int32_t cos_sin_is_f32,
                               int32_t rot_dim, int32_t interleaved,
                               const int32_t* slot_ids /* [T] or NULL */,
                               void* key_cache, void* value_cache,
                               int64_t n_tokens, int32_t n_heads, int32_t n_kv_heads,
                               int32_t head_dim, int32_t dtype, void* stream);
/* The same with q / k / v given as the split-K partial sums the fused qkv GEMM left behind
 * (SLM_W4_DEFER_REDUCE; GEMM row = [q | k | v], N = (n_heads + 2 n_kv_heads) * head_dim):
 * x := T(sum_s partials[s][t][col]) in the reduce kernel's own order, so the result is
 * bit-identical to "reduce, then slm_rope_kv_append" with one launch less.  q, k, v are OUTPUTS
 * here (q rotated, k rotated, v), k / v also go to their cache slot when slot_ids != NULL.
 * Needs cos_sin, rot_dim % 8 == 0, head_dim % 4 == 0 (SLM_ERR_UNSUPPORTED otherwise: reduce first). */
SLM_API int slm_rope_kv_append_splitk(const float* partials /* [n_splits, T, N] */, int32_t n_splits,
                                      void* q, int64_t q_token_stride, void* k, int64_t k_token_stride,
                                      void* v, int64_t v_token_stride, const int32_t* positions,
                                      const void* cos_sin, int32_t cos_sin_is_f32, int32_t rot_dim,
                                      int32_t interleaved, const int32_t* slot_ids /* or NULL */,
                                      void* key_cache, void* value_cache, int64_t n_tokens,
                                      int32_t n_heads, int32_t n_kv_heads, int32_t head_dim,
                                      int32_t dtype, void* stream);
SLM_API int slm_silu_mul(void* out /* [T, d] */, const void* x /* [T, 2d]: gate | up */,
                         int64_t n_tokens, int64_t d, int32_t dtype, void* stream);

/* ---- device-side input advance for the next decode step ----------------------
 * Replaces, for a steady decode batch (q_len = 1 per sequence), the per-step host rebuild + H2D
 * copies of Batch::prepare_model_input (engine/batch.cpp:97-255, model_runner.cpp:194-203):
 * updates the graph's static input buffers IN PLACE on the device so a captured step can be
 * replayed without touching the host.  For sequence b with len = positions[b] + 1 tokens cached:
 *     positions[b]       <- len                                   (batch.cpp:155)
 *     new_cache_slots[b] <- block_table[block_cu_lens[b] + len / B] + len % B
 *                                                 (Sequence::kv_cache_slots, sequence.cpp:303-317)
 *     kv_cu_lens[i]      <- kv_cu_lens[i] + i      for i = 0..n_seqs   (every length grows by 1)
 * The block table is persistent: the host appends a block's first-slot id only when a sequence
 * crosses a block boundary; a missing block (len / B >= blocks of b) sets *overflow_flag |= 1 and
 * clamps the slot to the sequence's last block (the step must then be discarded by the host).
 * q_cu_lens is unchanged.  block_size must be a power of two.  Bit-exact integer contract. */
SLM_API int slm_decode_advance(int32_t* positions /* [n_seqs] */, int32_t* kv_cu_lens /* [n_seqs+1] */,
                               int32_t* new_cache_slots /* [n_seqs] */,
                               const int32_t* block_table, const int32_t* block_cu_lens /* [n_seqs+1] */,
                               int32_t n_seqs, int32_t block_size, int32_t* overflow_flag /* [1], may be NULL */,
                               void* stream);

/* The same for ANY batch (prefill chunks, speculative-verify rows and decode rows mixed, sequences
 * joining or leaving between steps): the integer inputs of a step built on the device from two small
 * per-sequence arrays and the persistent block table, instead of the per-token host loops and the
 * H2D copy of the flattened table of Batch::prepare_model_input (engine/batch.cpp:97-255).
 * For sequence b with n_kv = kv_cached[b] tokens already in the cache and q = max(q_lens[b], 0) new ones:
 *     q_cu_lens[b+1]  = q_cu_lens[b]  + q                                   (batch.cpp:139-140)
 *     kv_cu_lens[b+1] = kv_cu_lens[b] + n_kv + q
 *     for j in [n_kv, n_kv + q), t = q_cu_lens[b] + (j - n_kv):
 *         positions[t]       = j                                            (batch.cpp:155)
 *         new_cache_slots[t] = block_table[block_cu_lens[b] + j / B] + j % B (sequence.cpp:303-317)
 *     commit != 0: kv_cached[b] += q afterwards         (Sequence::commit_kv_cache, batch.cpp:197)
 * Rows t in [q_cu_lens[n_seqs], n_tokens_padded) are the graph padding of batch.cpp:219-244:
 * position 0, slot 0.  A position without a block sets *overflow_flag |= 1 and is clamped to the
 * sequence's last block (slot 0 when the sequence has no block at all; the host then discards the
 * step).  More new tokens than n_tokens_padded rows sets *overflow_flag |= 2: the rows that fit are
 * written, the cache positions are NOT committed.  A sequence with q = 0 (no token budget
 * this step: the reference drops it from the batch, batch.cpp:113-117) stays in the arrays as an
 * empty row range; the attention kernels skip it.  The host keeps what only it can decide: which
 * sequences run, their token budgets (q_lens), block allocation (appending first-slot ids).
 * block_size must be a power of two.  Bit-exact integer contract; one launch, capture-safe. */
SLM_API int slm_build_step_inputs(const int32_t* q_lens /* [n_seqs] */, int32_t* kv_cached /* [n_seqs] */,
                                  const int32_t* block_table, const int32_t* block_cu_lens /* [n_seqs+1] */,
                                  int32_t n_seqs, int32_t block_size, int32_t n_tokens_padded, int32_t commit,
                                  int32_t* positions /* [n_tokens_padded] */, int32_t* q_cu_lens /* [n_seqs+1] */,
                                  int32_t* kv_cu_lens /* [n_seqs+1] */, int32_t* new_cache_slots /* [n_tokens_padded] */,
                                  int32_t* overflow_flag /* [1], may be NULL */, void* stream);

/* ========================================================================== */
/* 6. xGMI all-reduce fused with residual-add + RMSNorm    */
/*    replaces  ProcessGroupNCCL::allreduce  (ncclAllReduce SUM, in place)    */
/*              src/model_parallel/process_group.cpp:135-153                  */
/*    callers   reduce_from_model_parallel_region, model_parallel.cpp:33-44,  */
/*              from the row-parallel linears (qlinear_awq_marlin_impl.cpp    */
/*              :357-363), followed in the decoder layer by                   */
/*              kernel::rms_norm_residual (layernorm_kernels.cu:125).         */
/*                                                                            */
/* Two-shot all-reduce in ONE launch per rank over peer-mapped buffers: every */
/* rank owns ceil(M / world) consecutive ROWS of the [M, H] message; it reads */
/* its rows of every rank's partial sum over xGMI, adds them in fp32 in rank  */
/* order (so all ranks hold bit-identical results), rounds to T, optionally   */
/* applies   h = x + residual; residual = T(h); y = T(h * rsqrt(mean h^2 +    */
/* eps)) * weight   (normalization.h:42-52, same arithmetic as slm_rms_norm)  */
/* to those rows, publishes them in place in its own buffer, and after one    */
/* cross-rank flag barrier gathers every other rank's rows into `out`.  The   */
/* residual stream stays row-sharded: a rank only ever touches its own rows.  */
/* Synchronisation: per-workgroup monotonically increasing flags in           */
/* peer-writable UNCACHED signal blocks (no host involvement, no reset, graph */
/* replay safe); bounded spins (20 s) -- a peer that never arrives raises     */
/* SLM_AR_ERR_TIMEOUT in the signal block's error word instead of hanging.    */
/* ========================================================================== */
#define SLM_AR_MAX_RANKS 8
#define SLM_AR_MAX_BLOCKS 128
#define SLM_SHM_HANDLE_BYTES 64
#define SLM_AR_ERR_TIMEOUT 1

/* Host-side set-up helpers (init time only; these DO allocate / map and are not capture-safe):
 * peer-shareable device memory and its interprocess handles (hipIpcGetMemHandle /
 * hipIpcOpenMemHandle; one process per GPU).  uncached != 0 allocates fine-grained uncached
 * memory (required for signal blocks: peers write them while a local kernel polls).  The memory is
 * zero-filled.  The 64-byte handle is exchanged by the caller (torch.distributed, MPI, a pipe ...). */
SLM_API int slm_shm_alloc(void** ptr, size_t bytes, int32_t uncached);
SLM_API int slm_shm_free(void* ptr);
SLM_API int slm_shm_export(void* ptr, uint8_t handle[SLM_SHM_HANDLE_BYTES]);
SLM_API int slm_shm_import(const uint8_t handle[SLM_SHM_HANDLE_BYTES], void** ptr);
SLM_API int slm_shm_close(void* ptr);
/* Thread-per-GPU shape (all ranks in ONE process, the reference's: process_group.cpp:98-123): no
 * handles -- the raw pointers are valid everywhere once `device` may access `peer_device`.  No-op
 * (SLM_OK) when both are the same device or access is already enabled. */
SLM_API int slm_shm_enable_peer_access(int32_t device, int32_t peer_device);

/* bytes of one rank's signal block (allocate with slm_shm_alloc(..., uncached = 1)) */
SLM_API size_t slm_ar_signal_bytes(void);
/* host read of a signal block's sticky error word (synchronises the device; debugging / self-test) */
SLM_API int slm_ar_read_error(const void* own_signal, int32_t* err);

typedef struct slm_ar_args {
  int32_t rank, world;                 /* world in 2..SLM_AR_MAX_RANKS */
  void* signals[SLM_AR_MAX_RANKS];     /* signals[r]: rank r's signal block as mapped in THIS process */
  void* buffers[SLM_AR_MAX_RANKS];     /* buffers[r]: rank r's [M, H] T partial sums as mapped here;
                                          buffers[rank] is local and is overwritten (own rows) */
  void* out;                           /* [M, H] T, local: the reduced (fused: normalised) rows of
                                          every rank; may alias buffers[rank] (in-place all-reduce) */
  void* residual;                      /* fused: [M, H] T local residual stream, only this rank's
                                          rows are read and updated (ALL rows in one-shot mode:
                                          M <= world and out != buffers[rank], where every rank
                                          reduces every row itself behind a single barrier);
                                          NULL = plain all-reduce */
  const void* weight;                  /* fused: RMSNorm weight [H] T */
  float eps;
  int32_t dtype;                       /* slm_dtype */
  int64_t M, H;                        /* H % 8 == 0, H <= 16384 */
  int32_t end_barrier;                 /* != 0: also wait until every peer has finished reading this
                                          rank's buffer (needed when the SAME buffer is refilled by
                                          the next producer; alternate two buffers to avoid it) */
  int32_t reserved;
} slm_ar_args;

SLM_API int slm_allreduce(const slm_ar_args* args, void* stream);
/* Test hook: the work of ALL `world` ranks in one launch on one device (ranks[r] holds rank r's
 * argument block, every pointer local).  Runs exactly the device code of slm_allreduce; lets the
 * algorithm be verified on a single GPU. */
SLM_API int slm_allreduce_simulate(const slm_ar_args* ranks, int32_t world, void* stream);

/* ========================================================================== */
/* 7. Host policy: one lane or two for a pure-decode step (round 5)           */
/*    no reference counterpart -- the two half-batch lanes are this build's   */
/*    own schedule of the decoder stack (models/meta/llama.h:123-345 is one   */
/*    serial chain per step); DESIGN.md 3.6.  Pure host code, no device work: */
/*    ONE source of the rule for the Python mirror (decode.two_lane_split)    */
/*    and the C++ host step (slm::LlamaForCausalLMHip::lane_split).           */
/*    The rule: (a) hard conditions -- lanes_min != 0, a pure-decode batch in */
/*    the reference's graph-replay sense (q_max_seq_len == 1 and n_tokens ==  */
/*    n_seqs, model_runner.cpp:112-140), >= 64 tokens, one rank or a          */
/*    tensor-parallel rank whose reductions may run on two streams            */
/*    (tp_lanes_ok); (b) lanes_min > 0: every such batch of >= lanes_min      */
/*    tokens; (c) lanes_min < 0 (auto): a MEASUREMENT recorded for this model */
/*    geometry and batch size (slm_decode_lane_policy_record: the start-up    */
/*    probe's one-lane vs two-lane time at a context length; the nearest      */
/*    recorded length within a factor 1.5 decides), else the constants        */
/*    measured on one MI355X for Llama-3-8B shapes (96 <= T <= 256, >= 12 MiB */
/*    of K + V per sequence, KV bytes of the step >= 8 x the layer's weights).*/
/* ========================================================================== */
typedef struct slm_lane_query {
  int32_t n_tokens, n_seqs, q_max_seq_len, kv_max_seq_len;
  int32_t world_size;        /* tensor-parallel ranks                                        */
  int32_t tp_lanes_ok;       /* world_size > 1: != 0 if the reductions may run on two streams */
  int32_t lanes_min;         /* -1 auto, 0 never, N = every pure-decode batch of >= N tokens  */
  int32_t n_heads, n_kv_heads, head_dim;   /* per rank                                        */
  int64_t layer_weight_bytes;              /* packed weight bytes of one decoder layer, per rank */
  int32_t kv_elem_bytes;     /* bytes per KV element (2)                                      */
  int32_t reserved;
} slm_lane_query;
/* rows of lane 0 (a multiple of 32, about half the batch) when the step should run as two lanes, else 0 */
SLM_API int32_t slm_decode_lane_split(const slm_lane_query* q);
/* record a measurement for (geometry of q, n_tokens, kv_max_seq_len): time of the same layers as one lane
 * and as two.  Process-wide table (<= 256 entries, oldest replaced); thread-safe. */
SLM_API int slm_decode_lane_policy_record(const slm_lane_query* q, float one_lane_us, float two_lane_us);
SLM_API int slm_decode_lane_policy_clear(void);
/* 1 if a recorded measurement (not the constants) would decide q, else 0 */
SLM_API int32_t slm_decode_lane_policy_measured(const slm_lane_query* q);

/* ========================================================================== */
/* 8. Logits processing and sampling (one launch per call)                    */
/*    replaces  LogitsProcessor::create + Sampler::forward as Worker::        */
/*              execute_model runs them (src/engine/worker.cpp:154-187):      */
/*              kernel::apply_frequency_presence_penalty / apply_repetition_  */
/*              penalty / apply_temperature_penalty (src/kernels/sampling/    */
/*              penalty_kernels.cu:9-143), TopKTopPLogitsProcessor            */
/*              (src/sampling/logits_processor.h:224-284) and Sampler         */
/*              (src/sampling/sampler.cpp:19-70).                             */
/*    Per row r of logits [n_rows, vocab], all arithmetic in fp32 on the      */
/*    widened logits, rounded nowhere in between, in this order:              */
/*     1. for the first lens[r] entries j with counts[j] > 0 (padding beyond  */
/*        lens is never touched -- the GPU kernel's semantics; the CPU        */
/*        detail:: version of the reference also penalises padding id 0):     */
/*          l[id] -= (float)count * freq;  l[id] -= pres   (two roundings)    */
/*     2. for the first lens[r] ids:  l = l < 0 ? l * rep : l / rep           */
/*     3. l *= (1.0f / t)   (IEEE reciprocal, as the reference's kernel;      */
/*        t == 0 counts as 1)                                                 */
/*     4. top-k: k <= 0 or k >= vocab is off; keep the k largest              */
/*     5. top-p: p = softmax over the top-k survivors; in descending order    */
/*        keep rank j iff (mass ranked before j) <= top_p -- rank 0 always;   */
/*        top_p >= 1 is off.  The masses are summed in 64-bit fixed point     */
/*        (2^-40 units) with integer atomics: exact and order-independent.    */
/*     6. processed = l where kept, -inf elsewhere; probs = softmax(processed)*/
/*        do_sample[r] == 0: argmax(processed), else argmax(probs / E) with   */
/*        E_i ~ Exp(1) drawn for the survivors only                           */
/*     7. logprob = log_softmax(processed) at the token; top-n (n <= 20)      */
/*        values and ids of log_softmax(processed), descending                */
/*    Ties: every ordering (top-k, top-p, argmax, top-n) is stable by index:  */
/*    among equal values the lower vocab id ranks first (-0 == +0).           */
/*    RNG: counter-based and stateless (graph replay safe).  Philox4x32-10,  */
/*    key = seeds[r] (lo, hi words), counter = (lo32(i >> 2), hi32(i >> 2),  */
/*    positions[r], 0), output word i & 3 -- rocRAND's                        */
/*    philox4x32_10_engine(seed, positions[r], i).next().  With x that word:  */
/*    u = ((x >> 8) + 0.5) * 2^-24 and E = -ln(u), evaluated as -logf(u) for */
/*    u < 1/2 and -log1pf(-(1 - u)) above (both operands exact in fp32).     */
/*    A row's outputs depend only on its logits, parameters, seed and         */
/*    position: not on its row index, the batch, or eager vs graph replay.    */
/*    Bit-identical across repeats (no float atomics; fixed reduction order). */
/*    Logits are finite or -inf (a token an earlier slm_logits_process       */
/*    filtered): a -inf carries no mass, is never drawn, has logprob -inf and */
/*    ranks after every finite value, by id.  Each row needs one finite       */
/*    logit; +inf and NaN are not supported.  One 1024-thread workgroup per   */
/*    row.                                                                    */
/* ========================================================================== */
#define SLM_SAMPLE_MAX_TOP 20
typedef struct slm_sampling_args {
  const void* logits;               /* [n_rows, vocab], row stride logits_stride (elements)    */
  int64_t logits_stride;
  int32_t dtype;                    /* SLM_F16, SLM_BF16 or SLM_F32                              */
  int32_t n_rows;
  int32_t vocab;                    /* <= 2^22; <= 2^19 when a penalty is given                  */
  int32_t max_unique;               /* row stride of unique_ids / unique_counts                  */
  /* per-row parameters [n_rows], each NULL = neutral.  fp32: the reference holds them in the
   * logits dtype (sampling/parameters.h:42-67); a caller that wants its exact bits widens those. */
  const float* frequency_penalties;
  const float* presence_penalties;
  const float* repetition_penalties;
  const float* temperatures;
  const float* top_p;
  const int64_t* top_k;             /* LongTensor, as the reference                              */
  /* the penalised tokens: unique ids (int64, as the reference's tensors hold them; unique within a
   * row's first lens entries, ids outside [0, vocab) are skipped), counts, lens */
  const int64_t* unique_ids;        /* [n_rows, max_unique]                                      */
  const int32_t* unique_counts;     /* [n_rows, max_unique]   (needed by frequency / presence)   */
  const int32_t* unique_lens;       /* [n_rows]                                                  */
  const uint8_t* do_sample;         /* [n_rows] bool, NULL = all greedy                          */
  const uint64_t* seeds;            /* [n_rows], NULL = 0                                        */
  const int32_t* positions;         /* [n_rows] position of the row's last input token, NULL = 0 */
  /* outputs, each NULL = not wanted */
  int32_t* next_tokens;             /* [n_rows] (slm_sample: required)                           */
  void* processed;                  /* [n_rows, processed_stride] dtype: processed logits, rounded
                                       once; may be `logits` itself (in place)                   */
  int64_t processed_stride;
  float* probs;                     /* [n_rows, vocab] fp32, contiguous                          */
  float* logprobs;                  /* [n_rows]                                                  */
  float* top_logprobs;              /* [n_rows, n_top]                                           */
  int32_t* top_tokens;              /* [n_rows, n_top]                                           */
  int32_t n_top;                    /* 0 .. min(SLM_SAMPLE_MAX_TOP, vocab)                       */
  int32_t reserved;
  void* workspace;                  /* penalised values: slm_sample_workspace_bytes              */
  size_t workspace_bytes;
} slm_sampling_args;

/* scratch the call needs (0 without penalties); a pure function of host-side sizes */
SLM_API size_t slm_sample_workspace_bytes(const slm_sampling_args* a);
/* steps 1-7: next_tokens (+ the optional outputs).  SLM_ERR_INVALID_ARG: NULL logits / next_tokens,
 * n_top outside 0..20 or > vocab, a penalty without its ids / counts / lens, bad sizes;
 * SLM_ERR_UNSUPPORTED: dtype, vocab too large; SLM_ERR_WORKSPACE; n_rows == 0 is a no-op. */
SLM_API int slm_sample(const slm_sampling_args* a, void* stream);
/* steps 1-5 only: writes `processed` (required; do_sample / seeds / the other outputs are ignored).
 * In place with penalties alone it touches only the penalised entries -- the drop-in form of
 * kernel::apply_*_penalty, each rounding to the dtype when its call ends as the reference's do. */
SLM_API int slm_logits_process(const slm_sampling_args* a, void* stream);

/* ========================================================================== */
/* 9. Rejection sampling: validation of speculative drafts (two launches)     */
/*    replaces  RejectionSampler::forward / random_sample / greedy_sample     */
/*              (src/speculative/rejection_sampler.cpp:22-226) as             */
/*              SpeculativeEngine::validate calls them                        */
/*              (src/engine/speculative_engine.cpp:187-238).                  */
/*    Sequence s in [0, n_seqs) brings k draft tokens d_j (j < k) and target  */
/*    rows j = 0..k (logits form) or j = 0..k-1 (probability form).  All      */
/*    arithmetic is fp32 without contraction, on the widened target values.   */
/*    Per row j < k, with l = target[s, j, :]:                                */
/*     1. logits form: m = max_i l_i, S = sum_i expf(l_i - m) (accumulated    */
/*        with online rescaling in a fixed order: within a few ulp of the    */
/*        plain sum), p_i = expf(l_i - m) / S (IEEE division).                */
/*        probability form: p_i = target[s, j, i].                           */
/*     2. sampled sequence (do_sample[s] != 0): d = draft_token_ids[s, j],    */
/*        q_d = draft_probs[s, j, d], ratio = p_d / q_d (IEEE division);      */
/*        the row is ACCEPTED iff u < ratio -- NaN (0 / 0) rejects, q_d == 0  */
/*        with p_d > 0 accepts; d outside [0, vocab) rejects (nothing is read */
/*        at d).  u = uniform[s, j] when `uniform` is given, else             */
/*        u = ((x >> 8) + 0.5) * 2^-24 with                                   */
/*        x = philox_word(seed, positions[s] + j, stream 1, word 0).          */
/*     3. the RECOVERED token of a rejected sampled row:                      */
/*          argmax_i max(p_i - q_i, 0) / E_i,                                 */
/*        E_i = -ln(u_i) of x = philox_word(seed, positions[s] + j, stream 2, */
/*        i), evaluated exactly as section 8's E.  The reference's division   */
/*        by the clamped sum (rejection_sampler.cpp:162-166) is a common      */
/*        positive factor and is dropped.  A row of zeros gives token 0 (the  */
/*        reference's argmax over a zero row).                                */
/*     greedy sequence: t_j = argmax_i l_i; accepted iff t_j == d; token t_j. */
/*    Ties: every argmax and the top-n order are stable by index (the lower   */
/*    id wins; -0 == +0).  Target values are finite or -inf (a token that     */
/*    slm_logits_process filtered: probability 0).                            */
/*    Outputs: next_tokens[s, j < k] = d_j if accepted, else the recovered    */
/*    token (sampled) or t_j (greedy); next_tokens[s, k] = bonus_token_ids[s] */
/*    (copied as given, never checked against vocab).  Let f be the first     */
/*    rejected j, or k if none.  mask_out_rejected != 0: every entry after f  */
/*    is -1 (build_accepted_mask).  accepted_lens[s] = f + 1: the verify-row  */
/*    inputs of s whose KV entries stay valid (an addition: a captured loop   */
/*    advances kv_cached by it without reading tokens on the host).           */
/*    logprobs[s, j] (j = 0..k) = log_softmax(l_j) at the UNMASKED token of   */
/*    row j, as the reference takes it (a bonus id outside [0, vocab) gives   */
/*    NaN); top-n values / ids of log_softmax(l_j), descending.  Logits form  */
/*    only.                                                                   */
/*    RNG: Philox4x32-10 as section 8 with key seeds[s] and counter           */
/*    (lo32(i >> 2), hi32(i >> 2), positions[s] + j, stream), word i & 3 --   */
/*    rocRAND's philox4x32_10_engine(seed, pos | stream << 32, i).  Streams 1 */
/*    (acceptance) and 2 (race) never meet slm_sample's stream 0.  Outputs of */
/*    s depend only on its own inputs, seed and position: not on its index    */
/*    in the batch, the batch, or eager vs graph replay; bit-identical across */
/*    repeats (no float atomics, fixed reduction order).                      */
/*    Plan: launch 1, one workgroup per (s, row): rows 0..k-1 (+ row k when   */
/*    logprobs are wanted) stream once -- max, sum, greedy argmax, the        */
/*    acceptance decision (and top-n) -- into a 16-byte workspace record.     */
/*    Launch 2: the race.  Masked without logprobs: one workgroup per         */
/*    sequence races its first rejected row only; otherwise one per (s, j).   */
/* ========================================================================== */
#define SLM_REJECTION_MAX_K 16
typedef struct slm_rejection_args {
  int32_t n_seqs;
  int32_t k;                        /* draft tokens per sequence, 1..SLM_REJECTION_MAX_K         */
  int32_t vocab;                    /* <= 2^22                                                   */
  int32_t dtype;                    /* target: SLM_F16, SLM_BF16 or SLM_F32 (probability form:
                                       SLM_F32)                                                  */
  int32_t target_is_probs;          /* != 0: target holds fp32 probabilities of rows 0..k-1      */
  int32_t mask_out_rejected;
  const int32_t* draft_token_ids;   /* [n_seqs, k], contiguous                                  */
  const float* draft_probs;         /* [s, j, vocab] fp32 (slm_sample's `probs`); NULL = every
                                       sequence greedy (do_sample is not read)                   */
  int64_t draft_seq_stride, draft_row_stride;    /* elements: row stride >= vocab, seq stride >= 0 */
  const void* target;               /* [s, j, vocab]: logits rows 0..k or probabilities 0..k-1  */
  int64_t target_seq_stride, target_row_stride;  /* elements: row stride >= vocab, seq stride >= 0
                                       (inputs are only read: sequences may interleave, e.g. a
                                       [k + 1, n, vocab] buffer viewed as [n, k + 1, vocab])     */
  const int32_t* bonus_token_ids;   /* [n_seqs]                                                  */
  const uint8_t* do_sample;         /* [n_seqs] bool, NULL = all greedy                          */
  const uint64_t* seeds;            /* [n_seqs], NULL = 0                                        */
  const int32_t* positions;         /* [n_seqs] position of the input token of row 0, NULL = 0   */
  const float* uniform;             /* [n_seqs, k] contiguous: replaces the acceptance draw      */
  /* outputs */
  int32_t* next_tokens;             /* [n_seqs, k + 1] contiguous (required)                     */
  int32_t* accepted_lens;           /* [n_seqs]                                                  */
  float* logprobs;                  /* [n_seqs, k + 1]                                           */
  float* top_logprobs;              /* [n_seqs, k + 1, n_top]                                    */
  int32_t* top_tokens;              /* [n_seqs, k + 1, n_top]                                    */
  int32_t n_top;                    /* 0 .. min(SLM_SAMPLE_MAX_TOP, vocab)                       */
  int32_t reserved;
  void* workspace;                  /* slm_rejection_sample_workspace_bytes                      */
  size_t workspace_bytes;
} slm_rejection_args;

/* scratch the call needs; a pure function of host-side sizes (n_seqs, k) */
SLM_API size_t slm_rejection_sample_workspace_bytes(const slm_rejection_args* a);
/* SLM_ERR_INVALID_ARG: NULL draft_token_ids / target / bonus_token_ids / next_tokens, k outside
 * 1..16, n_top outside 0..20 or > vocab, top-n without both outputs, logprobs with target_is_probs,
 * a row stride < vocab or a negative sequence stride (target, or draft when given); SLM_ERR_UNSUPPORTED: dtype (or a non-fp32 probability target), vocab
 * > 2^22; SLM_ERR_WORKSPACE: missing or too small; n_seqs == 0 is a no-op. */
SLM_API int slm_rejection_sample(const slm_rejection_args* a, void* stream);

/* ========================================================================== */
/* 10. Mixture of experts: routing, block alignment, grouped GEMMs            */
/*    replaces  llm::kernel::topk_softmax                                     */
/*              src/kernels/moe/topk_softmax_kernel.cu:272-293,               */
/*              llm::kernel::grouped_topk_sigmoid                             */
/*              src/kernels/moe/grouped_topk_sigmoid_kernel.cu:280-315,       */
/*              llm::kernel::moe::permute_align_block / sum_out               */
/*              src/kernels/moe/align_block_kernel.cu:192-240, 242-272,       */
/*              and the grouped GEMM Sm80KernelGroupedGemm                    */
/*              src/kernels/gemm/ (A[m,k], W[e,n,k], rows gathered through    */
/*              sorted_token_idxes / expert_ids, output [m*topk, n]) -- here  */
/*              over int4 experts in the packed layout of section 3.          */
/*    One launch per entry point, on the given stream, no host sync, no       */
/*    allocation: every call is capture-safe.  No float atomics and a fixed   */
/*    order everywhere: repeated runs are bit-identical.  T = n_tokens,       */
/*    E = n_experts, k = topk, n_flat = T * k; a FLAT INDEX is t * k + j.     */
/*                                                                            */
/*  Routing.  logits [T, E] fp32 contiguous -> weights [T, k] fp32, indices   */
/*  [T, k] int32.  E a power of two <= 256 (the reference's limit,            */
/*  topk_softmax_kernel.cu:223-266), 1 <= k <= E; finite logits assumed.      */
/*  Every ordering is stable by index: among equal values the lower expert id */
/*  ranks first (-0 == +0).  Output j = 0..k-1 is in descending order.        */
/*   slm_moe_topk_softmax: the k largest LOGITS are selected (no arithmetic   */
/*    in the selection: the reference's softmax-then-top-k in exact           */
/*    arithmetic); weights = softmax over all E experts at the selected ones, */
/*    p = expf(x - max) / sum.  renormalize != 0: divided by the sum of the k */
/*    weights (added in order j = 0..k-1) -- Mixtral's rule; 0 = reference.   */
/*   slm_moe_grouped_topk_sigmoid (grouped_topk_sigmoid_ref,                  */
/*    grouped_topk_sigmoid_kernel_test.cu:25-75): s = 1 / (1 + expf(-x)),     */
/*    c = s + correction_bias; experts form n_expert_groups consecutive       */
/*    groups of E / n_expert_groups >= 2; group score = the sum of the two    */
/*    largest c of the group; the topk_group best groups are kept; top-k of c */
/*    inside the kept groups (k <= topk_group * group size);                  */
/*    weights = s[idx] * scaling_factor (the UNBIASED score).                 */
/*                                                                            */
/*  Alignment.  topk_ids [T, k] int32 -> sorted_token_idxes: experts in       */
/*  ascending order, each expert's flat indices in ASCENDING order (stricter  */
/*  than the reference, whose large path leaves the order to atomics), padded */
/*  to a multiple of block_size with the padding id n_flat; expert_ids: one   */
/*  entry per block of block_size entries; empty experts get no block;        */
/*  n_padded_tokens[0] = entries in use.  The kernel writes every entry of    */
/*  [0, n_padded) itself, padding included (no pre-fill needed); entries past */
/*  n_padded are unspecified but never written past the capacities below.     */
/*  Ids outside [0, E) are dropped.  E <= 1024; block_size in                 */
/*  {16, 32, 64, 128, 256}.  cu_sum (optional, [E + 1] int32): the padded     */
/*  start offset of every expert, as the reference's workspace holds it.      */
/*  Capacity (slm_moe_align_capacity): at most m = min(E, n_flat) experts are */
/*  non-empty and each adds at most block_size - 1 padding entries, so        */
/*    max_padded = floor((n_flat + m * (block_size - 1)) / block_size)        */
/*                 * block_size,   max_blocks = max_padded / block_size       */
/*  -- tighter than the reference test's n_flat + E * (block_size - 1) when   */
/*  n_flat < E.  A captured graph sizes its buffers with it once.             */
/*                                                                            */
/*  slm_moe_sum (sum_out): out[t, :] = T(sum_j in[t, j, :]) -- fp32, in order */
/*  j = 0..k-1, one rounding; any k >= 1; contiguous input and output.        */
/*  slm_moe_sum_add: out[t, :] = T(in[t, 0, :] + ... + in[t, k-1, :] +        */
/*  addend[t, :]) -- the same fp32 accumulation with one more contiguous      */
/*  [T, dim] row per token (the always-on shared experts' output) added LAST, */
/*  one rounding: bit-identical to slm_moe_sum over [T, k + 1, dim] with the  */
/*  addend as slot k, without the copy and without a separate add launch.     */
/*  out may alias addend.  Checks as slm_moe_sum, plus addend NULL ->         */
/*  SLM_ERR_INVALID_ARG and (dim % 8 == 0) a misaligned addend ->             */
/*  SLM_ERR_ALIGNMENT.                                                        */
/*                                                                            */
/*  Grouped GEMM.  For every 32-row block b with b * 32 < *n_padded_tokens    */
/*  (read on the device), e = expert_ids[b], and every non-padding            */
/*  idx = sorted_token_idxes[b * 32 + r] (0 <= idx < n_flat):                 */
/*     C[idx, :] = epilogue( A[idx / a_div, :] . dequant(W_e) )               */
/*  i.e. the align step must have run with block_size 32.  a_div = k when A   */
/*  is the token matrix [T, K] (gate_up), 1 when A is [n_flat, K] (down).     */
/*  W_e: the packed layout of slm_w4_prepack (SLM_W4_PAIRED included) at      */
/*  wq + e * wq_expert_stride, sz + e * sz_expert_stride (bytes, multiples of */
/*  16 / 4); one expert's tables < 4 GiB each (32-bit offsets inside an       */
/*  expert; the expert base is a 64-bit pointer).  Epilogue: plain;           */
/*  SLM_W4_SILU_MUL on paired weights (format must carry SLM_W4_PAIRED; C is  */
/*  [n_flat, N/2]), bit-identical to the plain grouped GEMM followed by       */
/*  slm_silu_mul; or row scale: T(acc * row_scale[idx]) -- the fp32           */
/*  accumulator times the routing weight, one rounding (not with SILU_MUL).   */
/*  Padding rows may load a clamped row of A and are never stored; blocks     */
/*  beyond n_padded return at once (the grid is max_blocks x ceil(N / 128)    */
/*  tiles of 32 x 128, no split-K, no workspace).  f16 / bf16; group_size 32, */
/*  64, a power of two >= 128, or K (per-channel); K % 128 == 0, N % 64 == 0; */
/*  GPTQ and AWQ.  SLM_ERR_UNSUPPORTED before any launch: perm (act-order),   */
/*  bias, the 8-bit formats, other shapes / dtypes.                           */
/*                                                                            */
/*  Dense grouped GEMM (slm_moe_gemm): the same aligned-list contract over    */
/*  unquantised experts -- the reference kernel's own form.                   */
/*     C[idx, :] = epilogue( A[idx / a_div, :] . W_e^T )                      */
/*  W_e = w + e * w_expert_stride (elements), [N, K] with row stride ldw: the */
/*  checkpoint layout W[e, n, k], k contiguous (nn.Linear.weight), no         */
/*  prepack.  Align block size 32, padding id n_flat; padding rows load a     */
/*  clamped row and are never stored; blocks beyond n_padded, or whose expert */
/*  id is outside [0, E), return at once; the grid is sized by max_blocks, so */
/*  one captured graph serves any routing.  No workspace, no float atomics,   */
/*  one wave per 32 x 32 tile over the whole K in a fixed order: repeats are  */
/*  bit-identical, and so is every launch shape -- the columns per workgroup  */
/*  (128, 64 or 32) are chosen from max_blocks, N and flags alone.  f16 /     */
/*  bf16, fp32 accumulation, one rounding at the store; K % 32 == 0,          */
/*  N % 32 == 0; lda, ldw >= K and ldc in elements, lda / ldw /               */
/*  w_expert_stride multiples of 8 and a / w 16-byte aligned (16-byte loads); */
/*  one expert (N * ldw elements) < 4 GiB: a 64-bit expert base, 32-bit       */
/*  offsets inside it.  Epilogue: plain; row scale T(acc * row_scale[idx]),   */
/*  one rounding; or SLM_MOE_SILU_MUL: rows [0, N/2) of W_e are the gate (w1) */
/*  and rows [N/2, N) the up projection (w3), concatenated, not interleaved;  */
/*  C is [n_flat, N/2] and c[idx, i] = T(silu(g) * u), g = T(acc gate i),     */
/*  u = T(acc up i): bit-identical to the plain call into [n_flat, N]         */
/*  followed by slm_silu_mul; needs (N/2) % 32 == 0, not with row_scale.      */
/*  Before any launch: SLM_ERR_INVALID_ARG on NULL / negative arguments,      */
/*  unknown flags, SILU_MUL with row_scale, a stride below its extent;        */
/*  SLM_ERR_UNSUPPORTED on other dtypes, K % 32, N % 32, (N/2) % 32 with      */
/*  SILU_MUL, the size limits; SLM_ERR_ALIGNMENT on misaligned pointers or    */
/*  strides; n_flat == 0 or max_blocks == 0 is a no-op.                       */
/* ========================================================================== */
SLM_API int slm_moe_topk_softmax(const float* logits /* [T, E] */, float* weights /* [T, k] */,
                                 int32_t* indices /* [T, k] */, int64_t n_tokens, int32_t n_experts,
                                 int32_t topk, int32_t renormalize, void* stream);
SLM_API int slm_moe_grouped_topk_sigmoid(const float* logits /* [T, E] */, const float* correction_bias /* [E] */,
                                         float* weights /* [T, k] */, int32_t* indices /* [T, k] */,
                                         int64_t n_tokens, int32_t n_experts, int32_t n_expert_groups,
                                         int32_t topk_group, int32_t topk, float scaling_factor, void* stream);

/* worst-case sizes of the align step's outputs; SLM_ERR_INVALID_ARG on n_flat < 0, E outside 1..1024 or a
 * block_size outside {16, 32, 64, 128, 256} */
SLM_API int slm_moe_align_capacity(int64_t n_flat, int32_t n_experts, int32_t block_size,
                                   int64_t* max_padded, int64_t* max_blocks);

typedef struct slm_moe_align_args {
  const int32_t* topk_ids;          /* [n_flat] = [T, k] contiguous                               */
  int32_t* sorted_token_idxes;      /* [sorted_capacity]                                          */
  int32_t* expert_ids;              /* [blocks_capacity]                                          */
  int32_t* n_padded_tokens;         /* [1]                                                        */
  int32_t* cu_sum;                  /* [n_experts + 1] or NULL                                    */
  int64_t n_flat;                   /* T * k, < 2^31 - 256                                        */
  int64_t sorted_capacity;          /* entries of sorted_token_idxes, >= max_padded               */
  int64_t blocks_capacity;          /* entries of expert_ids, >= max_blocks                       */
  int32_t n_experts;
  int32_t block_size;
} slm_moe_align_args;
SLM_API int slm_moe_align_block(const slm_moe_align_args* a, void* stream);

SLM_API int slm_moe_sum(void* out /* [T, dim] */, const void* in /* [T, k, dim] */, int64_t n_tokens,
                        int32_t topk, int64_t dim, int32_t dtype, void* stream);
/* (the parameter list on its own line, as slm_moe_gemm's below: tests/test_moe_cpu.py pins this section's first entry
 * points by the pattern "name(", and tests/test_mla_glue_cpu.py covers this one) */
SLM_API int slm_moe_sum_add
    (void* out /* [T, dim] */, const void* in /* [T, k, dim] */, const void* addend /* [T, dim] */, int64_t n_tokens,
     int32_t topk, int64_t dim, int32_t dtype, void* stream);

typedef struct slm_moe_gemm_args {
  const void* a;                    /* [n_flat / a_div, K] T, row stride lda (elements)           */
  const void* wq;                   /* expert 0's packed weights                                  */
  const void* sz;                   /* expert 0's packed scale / zero table                       */
  const int32_t* perm;              /* must be NULL (act-order experts: unsupported)              */
  const void* bias;                 /* must be NULL                                               */
  void* c;                          /* [n_flat, N] T (SILU_MUL: [n_flat, N/2]), row stride ldc    */
  const float* row_scale;           /* [n_flat] fp32 or NULL                                      */
  const int32_t* sorted_token_idxes;
  const int32_t* expert_ids;
  const int32_t* n_padded_tokens;   /* [1], read on the device                                    */
  int64_t wq_expert_stride;         /* bytes between experts' packed weights                      */
  int64_t sz_expert_stride;         /* bytes between experts' scale / zero tables                 */
  int64_t n_flat;                   /* rows of c = T * k; the padding id                          */
  int64_t K, N;
  int64_t lda, ldc;
  int64_t group_size;               /* K for per-channel                                          */
  int32_t a_div;                    /* >= 1                                                       */
  int32_t n_experts;
  int32_t max_blocks;               /* sizes the grid: slm_moe_align_capacity(n_flat, E, 32)      */
  int32_t dtype;
  int32_t format;                   /* slm_w4_format the experts were packed from (| SLM_W4_PAIRED) */
  int32_t flags;                    /* 0 or SLM_W4_SILU_MUL                                       */
} slm_moe_gemm_args;
SLM_API int slm_moe_w4a16_gemm(const slm_moe_gemm_args* a, void* stream);

#define SLM_MOE_SILU_MUL 2          /* slm_moe_gemm flags: gate | up rows, c is [n_flat, N/2]      */
typedef struct slm_moe_gemm_dense_args {
  const void* a;                    /* [n_flat / a_div, K] T, row stride lda (elements)           */
  const void* w;                    /* expert 0: [N, K] T, k contiguous, row stride ldw           */
  void* c;                          /* [n_flat, N] T (SILU_MUL: [n_flat, N/2]), row stride ldc    */
  const float* row_scale;           /* [n_flat] fp32 or NULL                                      */
  const int32_t* sorted_token_idxes;
  const int32_t* expert_ids;
  const int32_t* n_padded_tokens;   /* [1], read on the device                                    */
  int64_t w_expert_stride;          /* elements between experts, >= (N - 1) * ldw + K             */
  int64_t n_flat;                   /* rows of c = T * k; the padding id                          */
  int64_t K, N;
  int64_t lda, ldw, ldc;
  int32_t a_div;                    /* >= 1                                                       */
  int32_t n_experts;
  int32_t max_blocks;               /* sizes the grid: slm_moe_align_capacity(n_flat, E, 32)      */
  int32_t dtype;
  int32_t flags;                    /* 0 or SLM_MOE_SILU_MUL                                      */
} slm_moe_gemm_dense_args;
/* (the parameter list sits on its own line on purpose: tests/test_moe_cpu.py pins the entry points this section
 * had before slm_moe_gemm by the pattern "name(", and tests/test_moe_dense_cpu.py covers this one) */
SLM_API int slm_moe_gemm
    (const slm_moe_gemm_dense_args* a, void* stream);

/* ========================================================================== */
/* 11. Multi-head latent attention (MLA) over a paged latent KV cache         */
/*    mirrors   the reference's MLA kernel family                             */
/*              src/kernels/attention/mla_params.h (MLAPagedKVParams),        */
/*              device/sm80_mla_dispatch.cuh; semantics tests/mla_ref.h:      */
/*      S[q,k]     = sm_scale (q[q,h,:] . kv[k,:] + q_rope[q,h,:] . k_rope[k,:]) */
/*      S[q,k]     = -inf where k > q + (kv_len_b - q_len_b)                  */
/*      out[q,h,:] = softmax_k(S[q,:]) . kv[:, :]   (V IS the latent row)     */
/*    ONE latent row and one RoPE key per token, shared by all heads; both    */
/*    caches paged exactly as in section 1 (same block table for both).       */
/*    One entry point for decode, prefill, chunked prefill and verify.        */
/*    f16 / bf16; head_dim 128, 256 or 512; rope_head_dim 64; any n_heads >=  */
/*    1; block_size any power of two.  No soft-cap, alibi or sliding window   */
/*    (the reference's MLA has none).  Hints as in section 1: max_q_len       */
/*    bounds the query rows per sequence and sizes the grid; max_kv_len only  */
/*    sizes the KV splits -- results are correct for any value.  Lengths and  */
/*    tables are read on the device only, so a captured graph replays over    */
/*    changed ones.  A pure-decode call may carry more rows than              */
/*    q_cu_lens[batch] (graph padding): they are left untouched.              */
/*    Split-KV goes through the caller's workspace (fp32 partials, merged in  */
/*    split order by a combine pass: no atomics, repeats are bit-identical).  */
/*    Checked before any launch: null pointer / block_size not a power of two */
/*    -> SLM_ERR_INVALID_ARG; other head_dim / rope_head_dim / dtype ->       */
/*    SLM_ERR_UNSUPPORTED; a base or stride that is not 16-byte aligned ->    */
/*    SLM_ERR_ALIGNMENT; workspace missing or short -> SLM_ERR_WORKSPACE.     */
/*    batch_size == 0 or n_tokens == 0: SLM_OK without a launch.              */
/* ========================================================================== */
typedef struct slm_mla_args {
  void* out;                 /* [n_tokens, n_heads, head_dim]                  */
  const void* q;             /* [n_tokens, n_heads, head_dim]                  */
  const void* q_rope;        /* [n_tokens, n_heads, rope_head_dim]             */
  const void* kv_cache;      /* [n_slots, head_dim]                            */
  const void* k_rope_cache;  /* [n_slots, rope_head_dim]                       */
  int64_t o_stride[2];       /* {token stride, head stride} in elements        */
  int64_t q_stride[2];
  int64_t q_rope_stride[2];
  int64_t kv_stride;         /* slot stride of kv_cache in elements            */
  int64_t k_rope_stride;     /* slot stride of k_rope_cache                    */
  const int32_t* q_cu_lens;      /* [batch+1]                                  */
  const int32_t* kv_cu_lens;     /* [batch+1]                                  */
  const int32_t* block_table;    /* [sum_b ceil(kv_len_b / block_size)]        */
  const int32_t* block_cu_lens;  /* [batch+1]                                  */
  int32_t dtype;             /* slm_dtype of out / q / q_rope / caches         */
  int32_t batch_size;
  int32_t n_tokens;          /* rows of out / q / q_rope (>= q_cu_lens[batch]) */
  int32_t n_heads;
  int32_t head_dim;          /* width of the latent row: 128, 256 or 512       */
  int32_t rope_head_dim;     /* 64                                             */
  int32_t block_size;        /* power of two                                   */
  int32_t max_q_len;         /* scheduling hint, as in section 1               */
  int32_t max_kv_len;        /* scheduling hint: sizes the KV splits only      */
  float sm_scale;
  void* workspace;           /* split-KV scratch, may be NULL if bytes == 0    */
  size_t workspace_bytes;
  int32_t num_splits;        /* 0 = auto (heuristic); > 0 forces the split count */
  int32_t reserved;
} slm_mla_args;

/* Scratch needed for `a` (host-side sizes only; 0 without a KV split).  Pass num_splits to query a
 * forced split count. */
SLM_API size_t slm_mla_paged_kv_workspace_bytes(const slm_mla_args* a);
/* Split count the heuristic picks for `a` (host-side sizes only): 1 once the batch alone gives every
 * CU a workgroup. */
SLM_API int32_t slm_mla_paged_kv_auto_splits(const slm_mla_args* a);
SLM_API int slm_mla_paged_kv(const slm_mla_args* a, void* stream);

/* Latent cache append: kv_cache[slot_ids[t], :] = kv[t, :] and k_rope_cache[slot_ids[t], :] = k_rope[t, :]
 * in one launch (bit-exact copy; strides in elements, all 16-byte aligned; head_dim and rope_head_dim
 * multiples of 8).  A row whose slot id is negative (graph padding) is skipped; every other id must be a
 * valid slot of both caches. */
SLM_API int slm_mla_set_kv_cache(const int32_t* slot_ids /* [n_tokens] */, const void* kv /* [n_tokens, head_dim] */,
                                 const void* k_rope /* [n_tokens, rope_head_dim] */, int64_t kv_token_stride,
                                 int64_t k_rope_token_stride, void* kv_cache /* [n_slots, head_dim] */,
                                 void* k_rope_cache /* [n_slots, rope_head_dim] */, int64_t kv_slot_stride,
                                 int64_t k_rope_slot_stride, int64_t n_tokens, int32_t head_dim,
                                 int32_t rope_head_dim, int32_t dtype, void* stream);

/* ========================================================================== */
/* 12. Gemma family: Gemma RMSNorm (plain, sandwich, embedding) and soft cap  */
/*    mirrors   kernel::gemma_rms_norm  src/kernels/layernorm_kernels.cu:66   */
/*              (math src/layers/normalization.h:31-40), the layer of         */
/*              src/models/google/gemma2.h:186-204, its scaled embedding      */
/*              (:236-238,270) and its logit cap (:341-342)                   */
/*    GN(h, w)[i] = T(h[i] * rs * (1 + w[i])),  rs = rsqrt(mean(h^2) + eps):  */
/*    fp32 arithmetic and ONE rounding to T (f16 / bf16) at the end -- Gemma's */
/*    (x (1 + w)).to(T), not section 3's T(T(h rs) w).  h is always a row of  */
/*    T values.  One launch, one workgroup per token.  The form is chosen by  */
/*    which pointers are set:                                                 */
/*      A plain     x, pre_weight, out                                        */
/*                    out = GN(x, pre_weight)                                 */
/*      B sandwich  residual (in/out), x OR partials (+ n_splits),            */
/*                  post_weight (NULL: y = x, Gemma-1's plain residual        */
/*                  layer), pre_weight and out (both set or both NULL)        */
/*                    y = GN(x, post_weight); residual = T(y + residual);     */
/*                    out = GN(residual, pre_weight)   (skipped when NULL)    */
/*                  partials = fp32 split-K slabs [n_splits, n_tokens, dim]   */
/*                  of a deferred GEMM (SLM_W4_DEFER_REDUCE); x is then       */
/*                  T(sum of the slabs), summed and rounded exactly as the    */
/*                  reduce kernel and slm_rms_norm_splitk do                  */
/*      C embed     table [vocab, dim], token_ids [n_tokens], x_scale,        */
/*                  residual (output only), pre_weight, out                   */
/*                    residual = T(table[id] * x_scale);                      */
/*                    out = GN(residual, pre_weight)                          */
/*                  x_scale is used as the fp32 value given: pass a value of  */
/*                  T (Gemma: T(sqrt(hidden))) and the product is exact       */
/*                  before its rounding.  An id outside [0, vocab) is clamped */
/*                  into the table.                                           */
/*    out may be x.  Every other pointer combination: SLM_ERR_INVALID_ARG     */
/*    before any launch.  dim % 8 == 0 and dim <= 16384 and f16 / bf16, else  */
/*    SLM_ERR_UNSUPPORTED; every pointer 16-byte aligned (token_ids: 4), else */
/*    SLM_ERR_ALIGNMENT.  Rows at or beyond n_tokens are never written;       */
/*    n_tokens == 0 is SLM_OK without a launch.                               */
/* ========================================================================== */
typedef struct slm_gemma_norm_args {
  void* out;                 /* [n_tokens, dim]                                */
  const void* x;             /* [n_tokens, dim], or NULL                       */
  const float* partials;     /* [n_splits, n_tokens, dim] fp32, or NULL        */
  const void* post_weight;   /* [dim], or NULL                                 */
  const void* pre_weight;    /* [dim], or NULL (form B only)                   */
  void* residual;            /* [n_tokens, dim], or NULL (form A)              */
  const void* table;         /* [vocab, dim], or NULL                          */
  const int32_t* token_ids;  /* [n_tokens], or NULL                            */
  int64_t vocab;             /* rows of table (form C)                         */
  int64_t n_tokens;
  int64_t dim;
  int32_t n_splits;          /* slabs in partials                              */
  int32_t dtype;             /* slm_dtype of every 16-bit tensor               */
  float x_scale;             /* form C                                         */
  float eps;
} slm_gemma_norm_args;

SLM_API int slm_gemma_norm(const slm_gemma_norm_args* a, void* stream);

/* out = T(cap * tanh(x / cap)) over [n_rows, row_len] contiguous, in fp32 with ONE rounding to T.
 * The reference (gemma2.h:341-342) runs three element-wise ops on T and rounds three times (after the
 * division, after tanh, after the multiplication); this rounds once, so it is the closer of the two
 * to the real-valued function and differs from the reference in the last place of some elements.
 * tanh keeps a relative error of a few fp32 ulps at every magnitude (an odd polynomial below
 * |x / cap| = 0.25).  out == x (in place) is allowed.  cap must be positive and finite
 * (SLM_ERR_INVALID_ARG); row_len % 8 == 0 and f16 / bf16 (SLM_ERR_UNSUPPORTED); 16-byte aligned
 * pointers (SLM_ERR_ALIGNMENT); n_rows == 0 is SLM_OK without a launch. */
SLM_API int slm_soft_cap(void* out, const void* x, int64_t n_rows, int64_t row_len, float cap, int32_t dtype,
                         void* stream);

/* ========================================================================== */
/* 13. Dense linear: unquantised f16 / bf16 weights in checkpoint layout      */
/*    replaces  F::linear in {Column,Row}ParallelLinearImpl::forward          */
/*              src/layers/linear/parallel_linear.cpp (weight [out, in])      */
/*      C[M, N] = T( A[M, K] . W[N, K]^T + bias[N] )                          */
/*    fp32 accumulate, ONE rounding to T.  W is the checkpoint tensor [N, K], */
/*    k-contiguous, row stride ldw >= K, never prepacked; A has row stride    */
/*    lda, C row stride ldc (elements); every row 16-byte aligned.            */
/*    Shapes: K % 32 == 0, N % 32 == 0 (N % 64 with SLM_LINEAR_SILU_MUL), any */
/*    M >= 1, f16 / bf16: anything else SLM_ERR_UNSUPPORTED.  A null pointer  */
/*    or lda < K, ldw < K, ldc < output width: SLM_ERR_INVALID_ARG; all of it */
/*    before any launch.  M == 0 is SLM_OK without a launch.                  */
/*    Launch shape (csrc/dense.hip): one wave owns one 32-column tile over    */
/*    one K slice and `row_tiles` (1 / 2 / 4) 32-row accumulator tiles;       */
/*    `waves` (1 / 2 / 4, >= row_tiles) waves of a workgroup sit on adjacent  */
/*    column tiles and share the activation image in LDS.  Rows beyond        */
/*    32 * row_tiles go to further row blocks of the grid, which stream the   */
/*    weights again: correct at every M, tuned for decode (M <= 128) only.    */
/*    K split: split_k (1..16) contiguous ranges of whole 128-deep chunks of  */
/*    K, the K % 128 tail with the last; every slice writes an fp32 slab      */
/*    [M][N], slabs [split_k][M][N] at the START of `workspace`, summed in    */
/*    slice order by a second launch (+ bias, one rounding) -- or left to the */
/*    consumer (SLM_LINEAR_DEFER_REDUCE).  No atomics, no cross-workgroup     */
/*    hand-off.  split_k = the largest value that keeps row_blocks *          */
/*    col_groups * split_k <= 256 (the CUs) with >= 4 chunks per slice.       */
/*    Knobs: SLM_LINEAR_SPLITK, SLM_LINEAR_RT, SLM_LINEAR_NW (section 0).     */
/* ========================================================================== */
typedef struct slm_linear_args {
  const void* a;        /* [M, K] T, row stride lda                           */
  const void* w;        /* [N, K] T, row stride ldw                           */
  const void* bias;     /* [N] T or NULL                                      */
  void* c;              /* [M, N] T ([M, N/2] with SLM_LINEAR_SILU_MUL), row stride ldc */
  int64_t M, K, N;
  int64_t lda, ldw, ldc;
  int32_t dtype;
  int32_t flags;        /* SLM_LINEAR_* bits, 0 = none                        */
  void* workspace;      /* split-K slabs                                      */
  size_t workspace_bytes;
} slm_linear_args;

/* flags: as SLM_W4_DEFER_REDUCE -- a split call leaves its fp32 slabs at the start of `workspace`
 * and does NOT write c; ignored (normal reduce) when bias != NULL.  Ask slm_linear_deferred_splits. */
#define SLM_LINEAR_DEFER_REDUCE 1
/* flags: rows [0, N/2) of W are the gate, [N/2, N) the up projection and c is [M, N/2]:
 *   c[m, i] = T( silu(g) * u ),  g = T(acc[m, i] + bias[i]),  u = T(acc[m, N/2 + i] + bias[N/2 + i])
 * -- the bits of slm_linear into [M, N] followed by slm_silu_mul.  N % 64 == 0; never split over K;
 * cannot be combined with SLM_LINEAR_DEFER_REDUCE (SLM_ERR_INVALID_ARG). */
#define SLM_LINEAR_SILU_MUL 2
/* flags: scheduling hint as SLM_W4_SHARES_CHIP; accepted, the plan does not depend on it today. */
#define SLM_LINEAR_SHARES_CHIP 4

typedef struct slm_linear_plan_info {
  int32_t row_tiles;        /* 32-row accumulator tiles per wave: 1 / 2 / 4                         */
  int32_t waves;            /* waves (adjacent column tiles) per workgroup: 1 / 2 / 4               */
  int32_t row_blocks;       /* ceil(M / (32 * row_tiles))                                           */
  int32_t col_groups;       /* workgroups per row block and K slice                                 */
  int32_t split_k;          /* K slices, 1..16                                                      */
  int32_t n_chunks;         /* K / 128                                                              */
  int32_t tail_units;       /* (K % 128) / 32: consumed by the LAST slice                           */
  int32_t slice_chunk[17];  /* slice j covers chunks [slice_chunk[j], slice_chunk[j + 1])           */
  uint64_t lds_bytes;       /* static LDS of the launch                                             */
  uint64_t workspace_bytes; /* split_k * M * N * 4 when split_k > 1, else 0                         */
} slm_linear_plan_info;

/* The launch slm_linear gives `a`: a pure function of (M, N, K, dtype, flags, bias != NULL, tuning table);
 * no HIP call, works without a GPU.  The two queries below read from the same plan. */
SLM_API int slm_linear_plan(const slm_linear_args* a, slm_linear_plan_info* out);
SLM_API size_t slm_linear_workspace_bytes(const slm_linear_args* a);
/* number of slabs the call will leave in the workspace (>= 2), or 0 when it writes c as usual */
SLM_API int32_t slm_linear_deferred_splits(const slm_linear_args* a);
SLM_API int slm_linear(const slm_linear_args* a, void* stream);

/* ========================================================================== */
/* 14. MoE token permutation: tokens -> expert-major rows and back            */
/*    replaces  llm::kernel::moe::permute_with_index_map / _with_mask_map,    */
/*              unpermute_with_index_map / _with_mask_map                     */
/*              src/kernels/moe/permutation_index_kernel.cu, _mask_kernel.cu  */
/*    One map convention serves both forms: row_id_map is int32               */
/*    [n_maps, n_tokens], entry [m, t] = the row of the permuted tensor that  */
/*    holds token t for map slot m, or -1 for none.  n_maps = topk in the     */
/*    index form (slot = position in the token's id list) and n_experts in    */
/*    the mask form (slot = expert).  Permuted rows are expert-major; within  */
/*    an expert ascending flat index t * topk + j (index form: the stable     */
/*    sort of the flattened ids) or ascending token (mask form).              */
/*    The map entry points are one launch each, pure functions of their       */
/*    input (no atomic decides a position; counts use integer LDS atomics),   */
/*    read nothing on the host and can be captured.  n_experts <= 1024 and    */
/*    n_tokens * n_maps < 2^31 - 256, else SLM_ERR_INVALID_ARG, as a NULL     */
/*    input / map with n_tokens > 0.  n_tokens == 0 is SLM_OK; the counts,    */
/*    when given, are still zeroed.  Cost: every workgroup reads the whole    */
/*    input once and each expert's wave walks it again -- sized for decode    */
/*    and verify batches (a few thousand tokens); correct beyond.             */
/*    Row entry points: rows are contiguous, dim * sizeof(T) % 16 == 0 (else  */
/*    SLM_ERR_UNSUPPORTED, as any dtype but F16 / BF16 / F32); 1 <= n_maps    */
/*    <= 1024; negative sizes or a NULL pointer SLM_ERR_INVALID_ARG; row      */
/*    bases 16-byte aligned, else SLM_ERR_ALIGNMENT; all before any launch.   */
/*    n_tokens == 0 is SLM_OK without a launch.  Map entries that are         */
/*    negative or >= permuted_rows are skipped, so nothing outside            */
/*    permuted [permuted_rows, dim] is touched whatever the map holds.        */
/*    One wave owns 4 KiB of one token's row (csrc/permute.hip).              */
/* ========================================================================== */
/* topk_ids [n_tokens, topk] -> row_id_map [topk, n_tokens]; ids outside [0, n_experts) get -1 and take no row
 * (as slm_moe_align_block drops them).  tokens_per_expert [n_experts] or NULL: rows per expert. */
SLM_API int slm_permute_index_map(const int32_t* topk_ids, int64_t n_tokens, int32_t topk, int32_t n_experts,
                                  int32_t* row_id_map, int32_t* tokens_per_expert, void* stream);
/* routing_map [n_tokens, n_experts] bytes (non-zero = routed) -> row_id_map [n_experts, n_tokens].
 * tokens_per_expert [n_experts] or NULL; n_permuted [1] or NULL: the number of mapped rows. */
SLM_API int slm_permute_mask_map(const uint8_t* routing_map, int64_t n_tokens, int32_t n_experts,
                                 int32_t* row_id_map, int32_t* tokens_per_expert, int32_t* n_permuted, void* stream);
/* permuted[row_id_map[m, t]] = tokens[t] for every mapped m: a source row is read once, in 16-byte vectors.
 * permuted_rows == 0 stores nothing (SLM_OK without a launch). */
SLM_API int slm_permute_rows(void* permuted, const void* tokens, const int32_t* row_id_map, int64_t n_tokens,
                             int32_t n_maps, int64_t dim, int64_t permuted_rows, int32_t dtype, void* stream);
/* out[t] = T( sum_m probs[t, m] * permuted[row_id_map[m, t]] ): fp32 fma chain in ascending m over the mapped m,
 * ONE rounding (slm_moe_sum's convention; the reference accumulates in T).  probs [n_tokens, n_maps]
 * of probs_dtype = SLM_F32 or `dtype`, or NULL for 1.  A token with no mapped row gets zeros. */
SLM_API int slm_unpermute_rows(void* out, const void* permuted, const int32_t* row_id_map, const void* probs,
                               int32_t probs_dtype, int64_t n_tokens, int32_t n_maps, int64_t dim,
                               int64_t permuted_rows, int32_t dtype, void* stream);

/* ========================================================================== */
/* 15. fp8 (e4m3) weight-only linear: W8A16 over checkpoint-layout weights    */
/*    replaces  marlin::fp8_gemm  src/kernels/quantization/marlin.h:39-43     */
/*    (which reads a Marlin-repacked B; this entry reads the checkpoint       */
/*    tensor as it is, like section 13)                                       */
/*      acc_s[m, n] = sum over k in K slice s of A[m, k] * e4m3(W[n, k])      */
/*                    (e4m3 -> T is exact; fp32 MFMA accumulation, the order  */
/*                    of section 13 under the same plan)                      */
/*      y_s[m, n]   = acc_s[m, n] * w_scale[n]     ONE fp32 multiply, never   */
/*                    contracted into the bias add                            */
/*      C[m, n]     = T( y_0 + y_1 + ... (slice order) + bias[n] )   ONE      */
/*                    rounding to T                                           */
/*    W is [N, K] BYTES in OCP e4m3fn (torch.float8_e4m3fn; not the fnuz      */
/*    form), k-contiguous, never prepacked; row stride ldw in elements =      */
/*    bytes, ldw >= K, ldw % 16 == 0, base 16-byte aligned.  w_scale is fp32  */
/*    [N] (16-byte aligned), NULL = 1.0: one scale per output channel; the    */
/*    host expands a per-tensor scale (the q | k | v or gate | up shards of a */
/*    fused layer each bring their own).  No group / block scale and no       */
/*    activation scale (a checkpoint's input_scale is not used: W8A16).       */
/*    The two NaN codes 0x7F / 0xFF convert to NaN of T (the hardware         */
/*    converter propagates them) and poison their output column like a NaN    */
/*    weight of section 13 would; checkpoints do not hold them.               */
/*    A, bias, C are T (f16 / bf16), lda / ldc as in section 13.  Shapes,     */
/*    error codes, "all validation before any launch", M == 0, the launch     */
/*    shape, the K slices (whole 128-deep chunks, the K % 128 tail with the   */
/*    last), the workspace ([split_k][M][N] fp32 slabs, here ALREADY scaled,  */
/*    so the reduce launch and every deferred consumer of section 13 work     */
/*    unchanged) and the flags (SLM_LINEAR_*, the same bits) are section      */
/*    13's.  With SLM_LINEAR_SILU_MUL  g = T(y + bias), u = T(y' + bias'):    */
/*    the bits of the plain call followed by slm_silu_mul.                    */
/*    Knobs: SLM_LINEAR_SPLITK / _RT / _NW force the form of this entry too;  */
/*    it has none of its own (csrc/dense.hip).                                */
/* ========================================================================== */
typedef struct slm_fp8_linear_args {
  const void* a;        /* [M, K] T, row stride lda                           */
  const void* w;        /* [N, K] e4m3fn bytes, row stride ldw                */
  const void* bias;     /* [N] T or NULL                                      */
  void* c;              /* [M, N] T ([M, N/2] with SLM_LINEAR_SILU_MUL), row stride ldc */
  int64_t M, K, N;
  int64_t lda, ldw, ldc;
  int32_t dtype;        /* of a, bias and c                                   */
  int32_t flags;        /* SLM_LINEAR_* bits, 0 = none                        */
  void* workspace;      /* split-K slabs                                      */
  size_t workspace_bytes;
  const float* w_scale; /* [N] fp32 or NULL (= 1.0); everything above is slm_linear_args, field for field */
} slm_fp8_linear_args;

/* As slm_linear_plan / _workspace_bytes / _deferred_splits / slm_linear (section 13) for the fp8 entry; the plan is
 * a pure host function and works without a GPU. */
SLM_API int slm_fp8_linear_plan(const slm_fp8_linear_args* a, slm_linear_plan_info* out);
SLM_API size_t slm_fp8_linear_workspace_bytes(const slm_fp8_linear_args* a);
SLM_API int32_t slm_fp8_linear_deferred_splits(const slm_fp8_linear_args* a);
SLM_API int slm_fp8_linear(const slm_fp8_linear_args* a, void* stream);

/* ========================================================================== */
/* 16. fp8 (e4m3) mixture-of-experts: grouped W8A16 GEMM                      */
/*    slm_moe_gemm (section 10) with section 15's weight side.  For every     */
/*    32-row block b of the aligned token list (slm_moe_align_block with      */
/*    block_size 32), e = expert_ids[b], idx = sorted[b * 32 + r]:            */
/*      acc[idx, n] = sum over k of A[idx / a_div, k] * e4m3(W_e[n, k])       */
/*                    (e4m3 -> T is exact; fp32 MFMA accumulation in          */
/*                    slm_moe_gemm's k order: on the same T values the        */
/*                    accumulators are slm_moe_gemm's bit for bit)            */
/*      y[idx, n]   = acc[idx, n] * w_scale[e, n]        ONE fp32 multiply    */
/*      C[idx, n]   = T( y * row_scale[idx] )            ONE rounding to T    */
/*    W_e = w + e * w_expert_stride BYTES, [N, K] bytes in OCP e4m3fn         */
/*    (torch.float8_e4m3fn), k contiguous, row stride ldw in bytes: the       */
/*    checkpoint tensor, never prepacked.  w_scale is fp32, one scale per     */
/*    expert and output channel at w_scale[e * w_scale_expert_stride + n];    */
/*    NULL = 1.0 (no multiply); the host expands a per-tensor scale (the      */
/*    gate and up rows of a merged weight each bring their own).  No block    */
/*    scale and no activation scale (W8A16).  The NaN codes 0x7F / 0xFF       */
/*    poison their output column as in section 15.                            */
/*    With SLM_MOE_SILU_MUL: g = T(y gate), u = T(y up), each under its own   */
/*    channel scale, c[idx, i] = T(silu(g) * u): the bits of the plain call   */
/*    followed by slm_silu_mul.  Not with row_scale.                          */
/*    The aligned-list contract, dead blocks (beyond n_padded, expert ids     */
/*    outside [0, E)), padding rows, the launch shape (128 / 64 / 32 columns  */
/*    per workgroup from max_blocks, N and flags alone; no split-K, no        */
/*    workspace, no atomics: bit-identical repeats and launch shapes), the    */
/*    shapes (K % 32 == 0, N % 32 == 0, (N/2) % 32 == 0 with SILU_MUL) and    */
/*    the error codes are slm_moe_gemm's, rule for rule.  The weight side:    */
/*    w 16-byte aligned, ldw % 16 == 0, w_expert_stride % 16 == 0, w_scale    */
/*    4-byte aligned (SLM_ERR_ALIGNMENT); ldw >= K, w_expert_stride >=        */
/*    (N - 1) * ldw + K, w_scale_expert_stride >= N when w_scale is given     */
/*    (SLM_ERR_INVALID_ARG); one expert (N * ldw bytes) < 4 GiB               */
/*    (SLM_ERR_UNSUPPORTED).  All validation before any launch; n_flat == 0   */
/*    or max_blocks == 0 is a no-op.                                          */
/* ========================================================================== */
typedef struct slm_moe_fp8_gemm_args {
  const void* a;                    /* [n_flat / a_div, K] T, row stride lda (elements)           */
  const void* w;                    /* expert 0: [N, K] float8_e4m3fn bytes, row stride ldw (bytes) */
  const float* w_scale;             /* [n_experts, N] fp32, expert stride w_scale_expert_stride, or NULL (1.0) */
  void* c;                          /* [n_flat, N] T (SILU_MUL: [n_flat, N/2]), row stride ldc    */
  const float* row_scale;           /* [n_flat] fp32 or NULL                                      */
  const int32_t* sorted_token_idxes;
  const int32_t* expert_ids;
  const int32_t* n_padded_tokens;   /* [1], read on the device                                    */
  int64_t w_expert_stride;          /* bytes between experts, >= (N - 1) * ldw + K                */
  int64_t w_scale_expert_stride;    /* floats between experts' scales, >= N                       */
  int64_t n_flat;                   /* rows of c = T * k; the padding id                          */
  int64_t K, N;
  int64_t lda, ldw, ldc;
  int32_t a_div;                    /* >= 1                                                       */
  int32_t n_experts;
  int32_t max_blocks;               /* sizes the grid: slm_moe_align_capacity(n_flat, E, 32)      */
  int32_t dtype;
  int32_t flags;                    /* 0 or SLM_MOE_SILU_MUL                                      */
} slm_moe_fp8_gemm_args;
/* (the parameter list on its own line, as slm_moe_gemm's: tests/test_moe_cpu.py pins section 10's first entry points
 * by the pattern "name(", and tests/test_moe_fp8_cpu.py covers this one) */
SLM_API int slm_moe_fp8_gemm
    (const slm_moe_fp8_gemm_args* a, void* stream);

/* ========================================================================== */
/* 17. Fused MoE router: gate GEMM + routing in one launch                    */
/*    For every token t:                                                      */
/*      logit[t, e] = sum over h of x[t, h] * gate_w[e, h]                    */
/*                    (a product of two T values is exact in fp32; fp32 MFMA  */
/*                    accumulation, never rounded to T)                       */
/*      weights[t, :k], indices[t, :k] = section 10's routing of logit[t, :]  */
/*                    scoring 0: slm_moe_topk_softmax (renormalize),          */
/*                    scoring 1: slm_moe_grouped_topk_sigmoid                 */
/*                    (correction_bias, n_expert_groups, topk_group,          */
/*                    scaling_factor)                                         */
/*      logits_out[t, :E] = logit[t, :] (fp32, contiguous) when not NULL.     */
/*    x is [T, hidden] T with row stride ldx, gate_w is gate.weight as the    */
/*    checkpoint holds it, [E, hidden] T with row stride ldw: no transpose,   */
/*    no fp32 copy.  The routing is section 10's own device code, so weights  */
/*    and indices are bit-identical to the section 10 entry run on            */
/*    logits_out, ties by the lower expert id included.                       */
/*    Batch invariance: the K split, the order of the additions and the tile  */
/*    position of a row depend on (hidden, E, dtype) alone, never on T, the   */
/*    row's index or the other rows: row t routed alone gives the bits it     */
/*    gives inside any batch; repeats are bit-identical; no float atomics.    */
/*    One launch on the given stream, no host sync, no allocation, no         */
/*    workgroup waits for another: capture-safe.  One workgroup owns 32       */
/*    token rows and all E columns; rows at or beyond T and experts at or     */
/*    beyond E inside a tile are loaded clamped and never stored.             */
/*    slm_moe_router_splits: the number of K slices a row tile is spread      */
/*    over, a pure function of (E, hidden, dtype) -- not of T.  This version  */
/*    always plans 1, which needs no workspace                                */
/*    (slm_moe_router_workspace_bytes gives 0); workspace / workspace_bytes   */
/*    are checked against that size.  Both helpers are host functions and     */
/*    launch nothing.                                                         */
/*    Limits: E a power of two <= 256, 1 <= k <= E, the grouped form under    */
/*    section 10's conditions; hidden % 32 == 0; f16 / bf16; ldx, ldw         */
/*    multiples of 8 and x, gate_w 16-byte aligned (16-byte loads).           */
/*    Before any launch: SLM_ERR_INVALID_ARG on NULL or negative arguments,   */
/*    an unknown scoring, a stride below hidden, correction_bias missing for  */
/*    scoring 1, the grouped conditions; SLM_ERR_UNSUPPORTED on other dtypes, */
/*    E or hidden outside the limits; SLM_ERR_ALIGNMENT on misaligned         */
/*    pointers or strides; SLM_ERR_WORKSPACE when the workspace is missing or */
/*    smaller than slm_moe_router_workspace_bytes; n_tokens == 0 is a no-op.  */
/* ========================================================================== */
typedef struct slm_moe_router_args {
  const void* x;                    /* [n_tokens, hidden] T, row stride ldx (elements)            */
  const void* gate_w;               /* [n_experts, hidden] T, row stride ldw (elements)           */
  const float* correction_bias;     /* [n_experts] fp32; NULL with scoring 0                      */
  float* weights;                   /* [n_tokens, topk] fp32, contiguous                          */
  int32_t* indices;                 /* [n_tokens, topk] int32, contiguous                         */
  float* logits_out;                /* [n_tokens, n_experts] fp32, contiguous, or NULL            */
  void* workspace;                  /* slm_moe_router_workspace_bytes, or NULL when that is 0     */
  int64_t workspace_bytes;
  int64_t n_tokens;
  int64_t hidden;
  int64_t ldx, ldw;
  int32_t n_experts;
  int32_t topk;
  int32_t dtype;
  int32_t scoring;                  /* 0 = softmax, 1 = grouped sigmoid                           */
  int32_t renormalize;              /* scoring 0                                                  */
  int32_t n_expert_groups;          /* scoring 1                                                  */
  int32_t topk_group;               /* scoring 1                                                  */
  float scaling_factor;             /* scoring 1                                                  */
} slm_moe_router_args;
/* (the parameter lists on their own lines, as slm_moe_gemm's: tests/test_moe_cpu.py pins section 10's first entry
 * points by the pattern "name(", and tests/test_moe_router_cpu.py covers these) */
SLM_API int slm_moe_router_splits
    (int32_t n_experts, int64_t hidden, int32_t dtype, int32_t* splits);
SLM_API int slm_moe_router_workspace_bytes
    (int64_t n_tokens, int32_t n_experts, int64_t hidden, int32_t dtype, size_t* bytes);
SLM_API int slm_moe_router
    (const slm_moe_router_args* a, void* stream);

/* ========================================================================== */
/* 18. MLA prologue: latent RMSNorm + RoPE + append into both caches          */
/*    What a DeepSeek-V2 layer does between its kv_a / q projection and       */
/*    section 11, in ONE launch.  For every token row t, with latent =        */
/*    latent_dim in {128, 256, 512}, rope = rope_head_dim = 64 (section 11's  */
/*    limits), nope = nope_head_dim, n_heads >= 0:                            */
/*      c    = kv_a[t, :latent],  k_pe = kv_a[t, latent : latent + rope]      */
/*      q[t, h, : nope + rope]    at q + t * q_token_stride + h (nope + rope) */
/*      n    = RMSNorm(c; norm_weight, eps), the statistic over the latent    */
/*             columns only, section 5's rounding (fp32 sum of squares,       */
/*             T(T(c rs) w)): BIT-IDENTICAL to slm_rms_norm on a contiguous   */
/*             copy of those columns (the same per-lane sums and the same     */
/*             wave reduction, shared through common.h);                      */
/*      k_pe and q[t, h, nope:] rotated by cos_sin[positions[t]] -- the row   */
/*             layout of section 5, [cos(32) | sin(32)], in T                 */
/*             (cos_sin_is_f32 = 0) or fp32; interleaved != 0 pairs           */
/*             (2i, 2i + 1) (HuggingFace's DeepSeek-V2), 0 pairs (i, i + 32): */
/*             BIT-IDENTICAL to slm_rope_kv_append on the same values with    */
/*             head_dim = rot_dim = 64 (rope.h holds the one spelling);       */
/*      slot = slot_ids[t] >= 0:  kv_cache[slot, :latent] = n,                */
/*             k_rope_cache[slot, :rope] = rotated k_pe (slot strides in      */
/*             elements, as slm_mla_set_kv_cache).  slot < 0 is graph         */
/*             padding: q is still rotated, neither cache is written.  Every  */
/*             other slot must be valid in both caches.                       */
/*    The rotated tails stay in q: section 11 reads them with q_rope =        */
/*    q + nope and strides {q_token_stride, nope + rope}.  kv_a is not        */
/*    modified.                                                               */
/*    slm_mla_rope_append (plain form): q is rotated IN PLACE, its nope       */
/*    columns are untouched; q may be NULL with n_heads = 0.  kv_a has its    */
/*    own pointer and token stride, so q and kv_a may be column slices of one */
/*    fused [q | latent | k_pe] GEMM output.                                  */
/*    slm_mla_rope_append_splitk (slab form): the inputs are the fp32 split-K */
/*    slabs [n_splits, T, N] a deferred slm_linear / slm_fp8_linear left      */
/*    behind (section 13), row = [q heads | latent | k_pe],                   */
/*    N = n_heads (nope + rope) + latent + rope; every value is               */
/*    T(sum_s partials[s][t][col]) in the reduce kernel's own slice order     */
/*    (splitk_sum4), so the result is bit-identical to "reduce, then the      */
/*    plain form".  q is an OUTPUT, written whole (nope columns included).    */
/*    f16 / bf16; nope % 8 == 0; every base and stride 16-byte aligned.  One  */
/*    launch on the given stream; no allocation, no host sync, no atomics, no */
/*    LDS or barrier, no workgroup waits for another: capture-safe, repeats   */
/*    are bit-identical.  positions and slot_ids are read on the device only, */
/*    so a captured launch replays over changed ones.                         */
/*    Before any launch: negative n_tokens / n_heads / nope, a NULL among     */
/*    kv_a (plain) / partials (slab; or n_splits < 1) / norm_weight /         */
/*    positions / cos_sin / slot_ids / kv_cache / k_rope_cache, q NULL with   */
/*    n_heads > 0 -> SLM_ERR_INVALID_ARG; other latent_dim / rope_head_dim /  */
/*    dtype, nope % 8 -> SLM_ERR_UNSUPPORTED; a base or stride that is not    */
/*    16-byte aligned -> SLM_ERR_ALIGNMENT.  n_tokens == 0 is a no-op.        */
/* ========================================================================== */
SLM_API int slm_mla_rope_append(void* q /* [T, n_heads, nope + rope] in place, or NULL */, int64_t q_token_stride,
                                const void* kv_a /* [T, latent + rope] */, int64_t kv_a_token_stride,
                                const void* norm_weight /* [latent] */, float eps,
                                const int32_t* positions /* [T] */, const void* cos_sin /* [max_pos, rope] */,
                                int32_t cos_sin_is_f32, int32_t interleaved, const int32_t* slot_ids /* [T] */,
                                void* kv_cache /* [n_slots, latent] */, void* k_rope_cache /* [n_slots, rope] */,
                                int64_t kv_slot_stride, int64_t k_rope_slot_stride, int64_t n_tokens,
                                int32_t n_heads, int32_t nope_head_dim, int32_t latent_dim, int32_t rope_head_dim,
                                int32_t dtype, void* stream);
SLM_API int slm_mla_rope_append_splitk(const float* partials /* [n_splits, T, N] */, int32_t n_splits,
                                       void* q /* [T, n_heads, nope + rope] out, or NULL */, int64_t q_token_stride,
                                       const void* norm_weight /* [latent] */, float eps,
                                       const int32_t* positions /* [T] */, const void* cos_sin /* [max_pos, rope] */,
                                       int32_t cos_sin_is_f32, int32_t interleaved, const int32_t* slot_ids /* [T] */,
                                       void* kv_cache /* [n_slots, latent] */, void* k_rope_cache /* [n_slots, rope] */,
                                       int64_t kv_slot_stride, int64_t k_rope_slot_stride, int64_t n_tokens,
                                       int32_t n_heads, int32_t nope_head_dim, int32_t latent_dim,
                                       int32_t rope_head_dim, int32_t dtype, void* stream);

/* ========================================================================== */
/* 19. QK-norm prologue: per-head q / k RMSNorm + RoPE + KV append            */
/*    What a Qwen3 / Qwen3-MoE layer does between its qkv projection and      */
/*    section 2's attention, in ONE launch.  For every token row t, every q   */
/*    head h < n_heads and every k head h < n_kv_heads, with D = head_dim in  */
/*    {64, 128, 256} and rot_dim == D (the whole head rotates):               */
/*      x    = q[t, h, :D] (at q + t * q_token_stride + h D) or k[t, h, :D]   */
/*      n    = RMSNorm(x; w, eps) over the head's D values, w = q_norm_weight */
/*             or k_norm_weight ([D], shared by all heads), section 5's       */
/*             rounding (fp32 sum of squares, T(T(x rs) w));                  */
/*      n rotated by cos_sin[positions[t]] -- section 5's row layout          */
/*             [cos(D/2) | sin(D/2)], in T (cos_sin_is_f32 = 0) or fp32;      */
/*             interleaved != 0 pairs (2i, 2i + 1), 0 pairs (i, i + D/2);     */
/*      q and k are written IN PLACE; slot = slot_ids[t] >= 0: k and v also   */
/*             go to key_cache / value_cache [n_slots, n_kv_heads, D]         */
/*             (dense slot rows, as slm_rope_kv_append).  slot < 0 is graph   */
/*             padding: q and k are still rotated in place, nothing is        */
/*             appended.  slot_ids == NULL skips the append.  v is only       */
/*             copied.                                                        */
/*    BIT-IDENTICAL to slm_rms_norm over contiguous copies of q viewed as     */
/*    [T * n_heads, D] rows and of k as [T * n_kv_heads, D] rows, followed by */
/*    slm_rope_kv_append (the per-lane sums, the wave reduction, rope_unit8:  */
/*    shared through common.h and rope.h).                                    */
/*    slm_qk_norm_rope_kv_append_splitk (slab form): the inputs are the fp32  */
/*    split-K slabs [n_splits, T, N] a deferred GEMM left behind (sections 3  */
/*    and 13), row = [q | k | v], N = (n_heads + 2 n_kv_heads) D; every value */
/*    is T(sum_s partials[s][t][col]) in the reduce kernel's slice order      */
/*    (splitk_sum4), so the result is bit-identical to "reduce, then the      */
/*    plain form".  q, k and v are OUTPUTS, as in                             */
/*    slm_rope_kv_append_splitk.                                              */
/*    f16 / bf16; token strides multiples of 8 elements, every base 16-byte   */
/*    aligned.  One launch on the given stream; no allocation, no host sync,  */
/*    no atomics, no LDS or barrier: capture-safe, repeats are bit-identical. */
/*    positions and slot_ids are read on the device only, so a captured       */
/*    launch replays over changed ones.                                       */
/*    Before any launch: negative n_tokens / head_dim / rot_dim, n_heads or   */
/*    n_kv_heads < 1, a NULL among q / k / v / q_norm_weight / k_norm_weight  */
/*    / positions / cos_sin, caches NULL with slot_ids given, partials NULL   */
/*    or n_splits < 1 (slab form) -> SLM_ERR_INVALID_ARG; other head_dim,     */
/*    rot_dim != head_dim, other dtypes -> SLM_ERR_UNSUPPORTED; a base or     */
/*    stride that is not 16-byte aligned -> SLM_ERR_ALIGNMENT.  n_tokens == 0 */
/*    is a no-op.                                                             */
/* ========================================================================== */
SLM_API int slm_qk_norm_rope_kv_append(void* q /* [T, n_heads, D] in place */, int64_t q_token_stride,
                                       void* k /* [T, n_kv_heads, D] in place */, int64_t k_token_stride,
                                       const void* v /* [T, n_kv_heads, D] */, int64_t v_token_stride,
                                       const void* q_norm_weight /* [D] */, const void* k_norm_weight /* [D] */,
                                       float eps, const int32_t* positions /* [T] */,
                                       const void* cos_sin /* [max_pos, rot_dim] */, int32_t cos_sin_is_f32,
                                       int32_t rot_dim, int32_t interleaved, const int32_t* slot_ids /* [T] or NULL */,
                                       void* key_cache, void* value_cache, int64_t n_tokens, int32_t n_heads,
                                       int32_t n_kv_heads, int32_t head_dim, int32_t dtype, void* stream);
SLM_API int slm_qk_norm_rope_kv_append_splitk(const float* partials /* [n_splits, T, N] */, int32_t n_splits,
                                              void* q /* out */, int64_t q_token_stride, void* k /* out */,
                                              int64_t k_token_stride, void* v /* out */, int64_t v_token_stride,
                                              const void* q_norm_weight /* [D] */,
                                              const void* k_norm_weight /* [D] */, float eps,
                                              const int32_t* positions /* [T] */,
                                              const void* cos_sin /* [max_pos, rot_dim] */, int32_t cos_sin_is_f32,
                                              int32_t rot_dim, int32_t interleaved,
                                              const int32_t* slot_ids /* [T] or NULL */, void* key_cache,
                                              void* value_cache, int64_t n_tokens, int32_t n_heads,
                                              int32_t n_kv_heads, int32_t head_dim, int32_t dtype, void* stream);

/* ========================================================================== */
/* 20. MXFP4 weight-only linear: W4A16 over OCP MX checkpoints                */
/*    Section 13's linear over weights in OCP Microscaling FP4: e2m1 elements */
/*    (1 sign, 2 exponent, 1 mantissa bit: 0, .5, 1, 1.5, 2, 3, 4, 6 and      */
/*    their negatives; no infinity, no NaN) with ONE e8m0 scale byte e per 32 */
/*    consecutive k, value 2^(e - 127).  The checkpoint tensors are read as   */
/*    they are (Quark `weight` / `weight_scale`, gpt-oss `*_blocks` /         */
/*    `*_scales`): no prepack, no group-size variants, no act-order.          */
/*      w[n, k]   = T( e2m1(W[n, k]) * 2^(e[n, k / 32] - 127) )               */
/*      C[m, n]   = T( sum_k A[m, k] * w[n, k] + bias[n] )    ONE rounding    */
/*    The block scale is applied by the hardware converter                    */
/*    (v_cvt_scalef32_pk_{bf16,f16}_fp4), never to the accumulator: it varies */
/*    along K.  e2m1 has one mantissa bit, so w[n, k] is EXACT wherever it is */
/*    zero or a normal number of T: bf16 for e in [2, 252], f16 for e in      */
/*    [114, 140] (0.5 * 2^-13 is f16's smallest normal, 6 * 2^13 is finite).  */
/*    There the MFMA sees exactly T(dequantised W) and, under the same plan,  */
/*    the call is slm_linear on that tensor bit for bit: fp32 accumulation in */
/*    section 13's order, the same slabs, the same epilogue.                  */
/*    Outside that range, as observed on an MI355X through this entry (one    */
/*    code per row, one-hot A) and pinned by tests/test_mxfp4_exact_gpu.py:   */
/*      * below it the converter rounds the exact product to nearest even     */
/*        into T's subnormals and keeps them (no flush): bf16 at e = 0 / 1    */
/*        still gives every product exactly (0.5 * 2^-127 = 2^-128 is a bf16  */
/*        subnormal); f16 at e = 100 gives 2^-24 for code 6.0 and 0 for the   */
/*        rest (round to nearest even of 6 * 2^-27), 0 for everything at      */
/*        e <= 2, exact subnormals at e = 112 / 113.  e = 0 is 2^-127: the    */
/*        converter reads the scale's exponent field, not the value +0.0.     */
/*      * above it a product beyond T's largest finite number is +-inf (bf16: */
/*        4 and 6 at e = 253, 2 .. 6 at e = 254; f16: 4 and 6 at e = 141,     */
/*        every non-zero code from e = 144 up), the other codes of the block  */
/*        stay exact and the zero codes stay 0.  An inf weight poisons its    */
/*        output column (inf * 0 = NaN in the MFMA).                          */
/*      * e = 255, the MX NaN, gives NaN for EVERY code, zero included, in    */
/*        both dtypes, and poisons the column like a NaN weight of section    */
/*        13.  Checkpoints hold none of these; padding may (and is not read). */
/*    W is [N, K/2] BYTES, a byte's LOW nibble is the lower k; row stride ldw */
/*    in bytes, ldw >= K/2, ldw % 16 == 0, base 16-byte aligned.  w_scale is  */
/*    [N, K/32] e8m0 bytes, REQUIRED (NULL is SLM_ERR_INVALID_ARG), row       */
/*    stride lds in bytes, lds >= K/32, no alignment of base or stride        */
/*    (K/32 is 21 at K = 672).  A, bias, C are T (f16 / bf16), lda / ldc as   */
/*    in section 13.  Shapes (K % 32 == 0, N % 32 == 0), error codes, "all    */
/*    validation before any launch", M == 0 (SLM_OK without a launch), the    */
/*    launch shape, the K slices, the workspace ([split_k][M][N] fp32 slabs,  */
/*    so the reduce launch and every deferred consumer of section 13 work     */
/*    unchanged) and the flags (SLM_LINEAR_*, the same bits) are section      */
/*    13's.  The plan is the dense plan of (M, N, K, dtype, flags, bias).     */
/*    There is no _workspace_bytes query: the size is                         */
/*    slm_linear_plan_info.workspace_bytes of slm_mxfp4_linear_plan.          */
/*    Knobs: SLM_LINEAR_SPLITK / _RT / _NW force the form of this entry too   */
/*    (csrc/dense.hip, csrc/mxfp4_cvt.h).                                     */
/* ========================================================================== */
typedef struct slm_mxfp4_linear_args {
  const void* a;        /* [M, K] T, row stride lda                           */
  const void* w;        /* [N, K/2] bytes of two e2m1 codes, row stride ldw (bytes) */
  const void* bias;     /* [N] T or NULL                                      */
  void* c;              /* [M, N] T ([M, N/2] with SLM_LINEAR_SILU_MUL), row stride ldc */
  int64_t M, K, N;
  int64_t lda, ldw, ldc;
  int32_t dtype;        /* of a, bias and c                                   */
  int32_t flags;        /* SLM_LINEAR_* bits, 0 = none                        */
  void* workspace;      /* split-K slabs                                      */
  size_t workspace_bytes;
  const uint8_t* w_scale; /* [N, K/32] e8m0 bytes, required; everything above is slm_linear_args, field for field */
  int64_t lds;          /* row stride of w_scale in bytes, >= K/32            */
} slm_mxfp4_linear_args;

/* As slm_linear_plan / _deferred_splits / slm_linear (section 13) for the MXFP4 entry; the plan is a pure host
 * function and works without a GPU. */
SLM_API int slm_mxfp4_linear_plan(const slm_mxfp4_linear_args* a, slm_linear_plan_info* out);
SLM_API int32_t slm_mxfp4_linear_deferred_splits(const slm_mxfp4_linear_args* a);
SLM_API int slm_mxfp4_linear(const slm_mxfp4_linear_args* a, void* stream);

/* ========================================================================== */
/* 21. MXFP4 mixture-of-experts: grouped W4A16 GEMM over OCP MX experts       */
/*    slm_moe_gemm (section 10) with section 20's weight side.  For every     */
/*    32-row block b of the aligned token list (slm_moe_align_block with      */
/*    block_size 32), e = expert_ids[b], idx = sorted[b * 32 + r]:            */
/*      w_e[n, k]   = T( e2m1(W_e[n, k]) * 2^(s_e[n, k / 32] - 127) )         */
/*      acc[idx, n] = sum over k of A[idx / a_div, k] * w_e[n, k]             */
/*      C[idx, n]   = T( acc * row_scale[idx] )          ONE rounding to T    */
/*    The block scale is applied by the hardware converter, never to the      */
/*    accumulator.  Where e2m1 * 2^(s - 127) is zero or a normal number of T  */
/*    (bf16: s in [2, 252]; f16: s in [114, 140]) w_e is exact and the call   */
/*    is slm_moe_gemm on the dequantised [E, N, K] tensor bit for bit (fp32   */
/*    MFMA accumulation in slm_moe_gemm's k order, the same launch shapes):   */
/*    the plain output, the row_scale form and the SLM_MOE_SILU_MUL form      */
/*    alike.  Scale bytes outside that range behave as section 20 says        */
/*    (subnormals kept, inf beyond T's range, s = 255 is NaN for every code). */
/*    W_e = w + e * w_expert_stride BYTES, [N, K/2] bytes of two e2m1 codes,  */
/*    a byte's LOW nibble the lower k, row stride ldw in bytes: the           */
/*    checkpoint tensor (Quark `weight`, gpt-oss `*_blocks`), never           */
/*    prepacked.  s_e = w_scale + e * w_scale_expert_stride BYTES, [N, K/32]  */
/*    e8m0 bytes, row stride lds in bytes; REQUIRED.                          */
/*    With SLM_MOE_SILU_MUL: rows [0, N/2) of W_e are the gate, [N/2, N) the  */
/*    up projection, c[idx, i] = T(silu(T(gate)) * T(up)): the bits of the    */
/*    plain call followed by slm_silu_mul.  Not with row_scale.               */
/*    The aligned-list contract, dead blocks (beyond n_padded, expert ids     */
/*    outside [0, E)), padding rows, the launch shape (128 / 64 / 32 columns  */
/*    per workgroup from max_blocks, N and flags alone; no split-K, no        */
/*    workspace, no atomics: bit-identical repeats and launch shapes), the    */
/*    shapes (K % 32 == 0, N % 32 == 0, (N/2) % 32 == 0 with SILU_MUL) and    */
/*    the error codes are slm_moe_gemm's, rule for rule.  The weight side:    */
/*    w 16-byte aligned, ldw % 16 == 0, w_expert_stride % 16 == 0             */
/*    (SLM_ERR_ALIGNMENT); ldw >= K/2, w_expert_stride >= (N - 1) * ldw +     */
/*    K/2, w_scale not NULL, lds >= K/32, w_scale_expert_stride >=            */
/*    (N - 1) * lds + K/32 (SLM_ERR_INVALID_ARG); w_scale, lds and            */
/*    w_scale_expert_stride carry no alignment requirement (K/32 is 21 at     */
/*    K = 672); one expert (N * ldw bytes, N * lds scale bytes) < 4 GiB       */
/*    (SLM_ERR_UNSUPPORTED).  No byte outside an expert's own [N, K/2] and    */
/*    [N, K/32] rows is read, so the padding of strided operands may hold     */
/*    anything.  All validation before any launch; n_flat == 0 or             */
/*    max_blocks == 0 is a no-op (csrc/moe_gemm.hip, csrc/mxfp4_cvt.h).       */
/* ========================================================================== */
typedef struct slm_moe_mxfp4_gemm_args {
  const void* a;                    /* [n_flat / a_div, K] T, row stride lda (elements)           */
  const void* w;                    /* expert 0: [N, K/2] bytes of two e2m1 codes, row stride ldw (bytes) */
  const uint8_t* w_scale;           /* expert 0: [N, K/32] e8m0 bytes, row stride lds (bytes); required */
  void* c;                          /* [n_flat, N] T (SILU_MUL: [n_flat, N/2]), row stride ldc    */
  const float* row_scale;           /* [n_flat] fp32 or NULL                                      */
  const int32_t* sorted_token_idxes;
  const int32_t* expert_ids;
  const int32_t* n_padded_tokens;   /* [1], read on the device                                    */
  int64_t w_expert_stride;          /* bytes between experts, >= (N - 1) * ldw + K/2              */
  int64_t w_scale_expert_stride;    /* bytes between experts' scales, >= (N - 1) * lds + K/32     */
  int64_t n_flat;                   /* rows of c = T * k; the padding id                          */
  int64_t K, N;
  int64_t lda, ldw, ldc;
  int32_t a_div;                    /* >= 1                                                       */
  int32_t n_experts;
  int32_t max_blocks;               /* sizes the grid: slm_moe_align_capacity(n_flat, E, 32)      */
  int32_t dtype;
  int32_t flags;                    /* 0 or SLM_MOE_SILU_MUL                                      */
  int64_t lds;                      /* row stride of w_scale in bytes, >= K/32; everything above is
                                       slm_moe_fp8_gemm_args, field for field (w_scale: bytes)    */
} slm_moe_mxfp4_gemm_args;
/* (the parameter list on its own line, as slm_moe_gemm's and slm_moe_fp8_gemm's; tests/test_moe_mxfp4_cpu.py covers
 * this entry) */
SLM_API int slm_moe_mxfp4_gemm
    (const slm_moe_mxfp4_gemm_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SLM_HIP_H_ */
