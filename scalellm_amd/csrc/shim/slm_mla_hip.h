// slm_mla_hip.h -- multi-head latent attention at the libtorch boundary, on top of the C ABI's section 11
// (include/slm_hip.h; csrc/mla.hip).
//
// The reference ships MLA as a kernel family (src/kernels/attention/mla_params.h, device/sm80_mla_dispatch.cuh)
// without a public free function, so nothing is added to the llm:: namespaces: slm::mla_paged_kv takes the argument
// list of the reference test's wrapper (mla_pagedkv_sm80, tests/sm80_mla_pagedkv_test.cu:28-39) plus the output
// tensor and the max_kv_len hint.  Everything runs on torch's current HIP stream; nothing synchronises with the host.
// Python mirror: scalellm_amd/kernels.py (same kernels, same arguments: bit-identical results).
#pragma once
#include <torch/torch.h>

namespace slm {

// out[q, h, :] = softmax_k(sm_scale (q . kv + q_rope . k_rope), causal) . kv over the paged latent cache.
// The split-KV scratch is ONE per-device buffer owned by the shim (grown outside graph capture only; run the call
// once before capturing it).  It is shared by every stream and thread: calls on one device must be stream-ordered
// (one stream, or ordered by events) -- two calls in flight at once on different streams would overwrite each
// other's partials.  The Python wrapper's workspace table has the same rule (kernels.workspace_lane separates lanes).
void mla_paged_kv(torch::Tensor& out,                  // [n_tokens, n_heads, head_dim]
                  const torch::Tensor& q,              // [n_tokens, n_heads, head_dim]
                  const torch::Tensor& kv_cache,       // [n_slots, head_dim]
                  const torch::Tensor& q_rope,         // [n_tokens, n_heads, rope_head_dim]
                  const torch::Tensor& k_rope_cache,   // [n_slots, rope_head_dim]
                  const torch::Tensor& q_cu_lens,      // [batch + 1] int32
                  const torch::Tensor& kv_cu_lens,     // [batch + 1] int32
                  const torch::Tensor& block_table,    // [n_blocks] int32
                  const torch::Tensor& block_cu_lens,  // [batch + 1] int32
                  int block_size, int max_q_len, int max_kv_len, float sm_scale);

// kv_cache[slot_ids[t]] = kv[t], k_rope_cache[slot_ids[t]] = k_rope[t] (bit-exact, one launch)
void mla_set_kv_cache(const torch::Tensor& slot_ids,  // [n_tokens] int32
                      const torch::Tensor& kv,        // [n_tokens, head_dim]
                      const torch::Tensor& k_rope,    // [n_tokens, rope_head_dim]
                      torch::Tensor& kv_cache,        // [n_slots, head_dim]
                      torch::Tensor& k_rope_cache);   // [n_slots, rope_head_dim]

// The MLA prologue of the C ABI's section 18 in one launch: the latent columns of kv_a RMS-normalised into
// kv_cache[slot], its rope columns rotated into k_rope_cache[slot], the last rope_head_dim columns of every head of q
// rotated in place.  q and kv_a may be column slices of one GEMM output; an undefined q means no query heads.  A
// negative slot id is graph padding: q is rotated, the caches are not written.  partials (defined): the fp32 split-K
// slabs [n_splits, n_tokens, N] of the fused [q | latent | k_pe] GEMM; kv_a is not used then and q is written whole.
void mla_rope_append(torch::Tensor q,                    // [n_tokens, n_heads, nope + rope] or undefined
                     const torch::Tensor& kv_a,          // [n_tokens, latent + rope] (undefined with partials)
                     const torch::Tensor& norm_weight,   // [latent]
                     double eps,
                     const torch::Tensor& positions,     // [n_tokens] int32
                     const torch::Tensor& cos_sin,       // [max_pos, rope], fp32 or the activation dtype
                     bool interleaved,
                     const torch::Tensor& slot_ids,      // [n_tokens] int32
                     torch::Tensor& kv_cache,            // [n_slots, latent]
                     torch::Tensor& k_rope_cache,        // [n_slots, rope]
                     int64_t nope_head_dim,
                     const torch::Tensor& partials = torch::Tensor());

// The QK-norm prologue of the C ABI's section 19 in one launch (Qwen3): every head of q and k RMS-normalised over its
// head_dim values with q_norm_weight / k_norm_weight, rotated over the whole head by cos_sin[positions], in place;
// with slot_ids defined, k and v also go to their cache slot (a negative id appends nothing).  q / k / v may be
// column slices of one GEMM output.  partials (defined): the fp32 split-K slabs [n_splits, n_tokens, N] of the fused
// [q | k | v] GEMM; q, k and v are then outputs.
void qk_norm_rope_kv_append(torch::Tensor q,                    // [n_tokens, n_heads, head_dim]
                            torch::Tensor k,                    // [n_tokens, n_kv_heads, head_dim]
                            torch::Tensor v,                    // [n_tokens, n_kv_heads, head_dim]
                            const torch::Tensor& q_norm_weight,  // [head_dim]
                            const torch::Tensor& k_norm_weight,  // [head_dim]
                            double eps,
                            const torch::Tensor& positions,      // [n_tokens] int32
                            const torch::Tensor& cos_sin,        // [max_pos, head_dim], fp32 or the activation dtype
                            bool interleaved,
                            const torch::Tensor& slot_ids = torch::Tensor(),     // [n_tokens] int32 or undefined
                            const torch::Tensor& key_cache = torch::Tensor(),    // [n_slots, n_kv_heads, head_dim]
                            const torch::Tensor& value_cache = torch::Tensor(),  // [n_slots, n_kv_heads, head_dim]
                            const torch::Tensor& partials = torch::Tensor());

}  // namespace slm
