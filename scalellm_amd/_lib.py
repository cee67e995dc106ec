"""ctypes binding of libslm_hip.so (the C-ABI HIP kernel library, include/slm_hip.h).

The product path FAILS LOUDLY when the HIP library is missing: there is no CPU or
PyTorch fallback anywhere in scalellm_amd (the CPU oracle under oracle/ is test
infrastructure and is never imported from here).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libslm_hip.so")

SLM_F16, SLM_BF16 = 0, 1
SLM_F32 = 2  # logits of the sampling entry points (slm_hip.h sections 8 / 9), token rows of section 14
SLM_SAMPLE_MAX_TOP = 20
SLM_REJECTION_MAX_K = 16
SLM_W4_GPTQ, SLM_W4_AWQ = 0, 1
SLM_W8_GPTQ, SLM_W8_AWQ = 2, 3  # 8-bit checkpoints: slm_w8_prepack_* (two int4 planes)
SLM_W4_PAIRED = 0x10


class SlmError(RuntimeError):
    pass


class AttnArgs(C.Structure):
    """struct slm_attn_args (include/slm_hip.h)."""
    _fields_ = [
        ("out", C.c_void_p), ("query", C.c_void_p), ("key_cache", C.c_void_p),
        ("value_cache", C.c_void_p),
        ("o_stride", C.c_int64 * 2), ("q_stride", C.c_int64 * 2), ("k_stride", C.c_int64 * 2),
        ("v_stride", C.c_int64 * 2),
        ("q_cu_lens", C.c_void_p), ("kv_cu_lens", C.c_void_p), ("block_table", C.c_void_p),
        ("block_cu_lens", C.c_void_p), ("alibi_slopes", C.c_void_p),
        ("dtype", C.c_int32), ("batch_size", C.c_int32), ("n_tokens", C.c_int32),
        ("n_heads", C.c_int32), ("n_kv_heads", C.c_int32), ("head_dim", C.c_int32),
        ("block_size", C.c_int32), ("max_q_len", C.c_int32), ("max_kv_len", C.c_int32),
        ("sm_scale", C.c_float), ("logits_soft_cap", C.c_float), ("sliding_window", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("num_splits", C.c_int32), ("total_kv_len", C.c_int32),
        ("phase", C.c_int32), ("n_slots", C.c_int32),
    ]


class W4GemmArgs(C.Structure):
    """struct slm_w4_gemm_args (include/slm_hip.h)."""
    _fields_ = [
        ("a", C.c_void_p), ("wq", C.c_void_p), ("sz", C.c_void_p), ("perm", C.c_void_p),
        ("bias", C.c_void_p), ("c", C.c_void_p),
        ("M", C.c_int64), ("K", C.c_int64), ("N", C.c_int64),
        ("lda", C.c_int64), ("ldc", C.c_int64), ("group_size", C.c_int64),
        ("dtype", C.c_int32), ("flags", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


SLM_W4_DEFER_REDUCE = 1
SLM_W4_SILU_MUL = 2
SLM_W4_SHARES_CHIP = 4

# enum slm_w4_kernel, in value order
W4_KERNELS = ("GEMV", "KS", "SMALL", "GENERAL", "M128", "WS", "XL", "XL_SK")


class W4PlanInfo(C.Structure):
    """struct slm_w4_plan_info (include/slm_hip.h)."""
    _fields_ = [
        ("kernel", C.c_int32), ("row_tiles", C.c_int32), ("n_mblocks", C.c_int32),
        ("n_nblocks", C.c_int32), ("split_k", C.c_int32), ("chunks_per_split", C.c_int32),
        ("variant", C.c_int32 * 4),
        ("lds_bytes", C.c_uint64), ("part_bytes", C.c_uint64), ("aperm_bytes", C.c_uint64),
    ]

    @property
    def kernel_name(self) -> str:
        return W4_KERNELS[self.kernel]


class W4NormPrologue(C.Structure):
    """struct slm_w4_norm_prologue (include/slm_hip.h)."""
    _fields_ = [
        ("x", C.c_void_p), ("partials", C.c_void_p), ("n_splits", C.c_int32), ("eps", C.c_float),
        ("residual_in", C.c_void_p), ("residual_out", C.c_void_p), ("weight", C.c_void_p),
        ("normed_out", C.c_void_p),
    ]


class LaneQuery(C.Structure):
    """slm_lane_query (include/slm_hip.h section 7)."""
    _fields_ = [("n_tokens", C.c_int32), ("n_seqs", C.c_int32), ("q_max_seq_len", C.c_int32),
                ("kv_max_seq_len", C.c_int32), ("world_size", C.c_int32), ("tp_lanes_ok", C.c_int32),
                ("lanes_min", C.c_int32), ("n_heads", C.c_int32), ("n_kv_heads", C.c_int32),
                ("head_dim", C.c_int32), ("layer_weight_bytes", C.c_int64), ("kv_elem_bytes", C.c_int32),
                ("reserved", C.c_int32)]


class ArArgs(C.Structure):
    """struct slm_ar_args (include/slm_hip.h)."""
    _fields_ = [
        ("rank", C.c_int32), ("world", C.c_int32),
        ("signals", C.c_void_p * 8), ("buffers", C.c_void_p * 8),
        ("out", C.c_void_p), ("residual", C.c_void_p), ("weight", C.c_void_p),
        ("eps", C.c_float), ("dtype", C.c_int32),
        ("M", C.c_int64), ("H", C.c_int64),
        ("end_barrier", C.c_int32), ("reserved", C.c_int32),
    ]


class SamplingArgs(C.Structure):
    """struct slm_sampling_args (include/slm_hip.h section 8)."""
    _fields_ = [
        ("logits", C.c_void_p), ("logits_stride", C.c_int64),
        ("dtype", C.c_int32), ("n_rows", C.c_int32), ("vocab", C.c_int32), ("max_unique", C.c_int32),
        ("frequency_penalties", C.c_void_p), ("presence_penalties", C.c_void_p),
        ("repetition_penalties", C.c_void_p), ("temperatures", C.c_void_p), ("top_p", C.c_void_p),
        ("top_k", C.c_void_p),
        ("unique_ids", C.c_void_p), ("unique_counts", C.c_void_p), ("unique_lens", C.c_void_p),
        ("do_sample", C.c_void_p), ("seeds", C.c_void_p), ("positions", C.c_void_p),
        ("next_tokens", C.c_void_p), ("processed", C.c_void_p), ("processed_stride", C.c_int64),
        ("probs", C.c_void_p), ("logprobs", C.c_void_p), ("top_logprobs", C.c_void_p),
        ("top_tokens", C.c_void_p), ("n_top", C.c_int32), ("reserved", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class RejectionArgs(C.Structure):
    """struct slm_rejection_args (include/slm_hip.h section 9)."""
    _fields_ = [
        ("n_seqs", C.c_int32), ("k", C.c_int32), ("vocab", C.c_int32), ("dtype", C.c_int32),
        ("target_is_probs", C.c_int32), ("mask_out_rejected", C.c_int32),
        ("draft_token_ids", C.c_void_p), ("draft_probs", C.c_void_p),
        ("draft_seq_stride", C.c_int64), ("draft_row_stride", C.c_int64),
        ("target", C.c_void_p), ("target_seq_stride", C.c_int64), ("target_row_stride", C.c_int64),
        ("bonus_token_ids", C.c_void_p), ("do_sample", C.c_void_p), ("seeds", C.c_void_p),
        ("positions", C.c_void_p), ("uniform", C.c_void_p),
        ("next_tokens", C.c_void_p), ("accepted_lens", C.c_void_p), ("logprobs", C.c_void_p),
        ("top_logprobs", C.c_void_p), ("top_tokens", C.c_void_p), ("n_top", C.c_int32), ("reserved", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class MoeAlignArgs(C.Structure):
    """struct slm_moe_align_args (include/slm_hip.h section 10)."""
    _fields_ = [
        ("topk_ids", C.c_void_p), ("sorted_token_idxes", C.c_void_p), ("expert_ids", C.c_void_p),
        ("n_padded_tokens", C.c_void_p), ("cu_sum", C.c_void_p),
        ("n_flat", C.c_int64), ("sorted_capacity", C.c_int64), ("blocks_capacity", C.c_int64),
        ("n_experts", C.c_int32), ("block_size", C.c_int32),
    ]


class MoeGemmArgs(C.Structure):
    """struct slm_moe_gemm_args (include/slm_hip.h section 10)."""
    _fields_ = [
        ("a", C.c_void_p), ("wq", C.c_void_p), ("sz", C.c_void_p), ("perm", C.c_void_p), ("bias", C.c_void_p),
        ("c", C.c_void_p), ("row_scale", C.c_void_p),
        ("sorted_token_idxes", C.c_void_p), ("expert_ids", C.c_void_p), ("n_padded_tokens", C.c_void_p),
        ("wq_expert_stride", C.c_int64), ("sz_expert_stride", C.c_int64), ("n_flat", C.c_int64),
        ("K", C.c_int64), ("N", C.c_int64), ("lda", C.c_int64), ("ldc", C.c_int64), ("group_size", C.c_int64),
        ("a_div", C.c_int32), ("n_experts", C.c_int32), ("max_blocks", C.c_int32), ("dtype", C.c_int32),
        ("format", C.c_int32), ("flags", C.c_int32),
    ]


class MoeDenseGemmArgs(C.Structure):
    """struct slm_moe_gemm_dense_args (include/slm_hip.h section 10)."""
    _fields_ = [
        ("a", C.c_void_p), ("w", C.c_void_p), ("c", C.c_void_p), ("row_scale", C.c_void_p),
        ("sorted_token_idxes", C.c_void_p), ("expert_ids", C.c_void_p), ("n_padded_tokens", C.c_void_p),
        ("w_expert_stride", C.c_int64), ("n_flat", C.c_int64), ("K", C.c_int64), ("N", C.c_int64),
        ("lda", C.c_int64), ("ldw", C.c_int64), ("ldc", C.c_int64),
        ("a_div", C.c_int32), ("n_experts", C.c_int32), ("max_blocks", C.c_int32), ("dtype", C.c_int32),
        ("flags", C.c_int32),
    ]


class MoeFp8GemmArgs(C.Structure):
    """struct slm_moe_fp8_gemm_args (include/slm_hip.h section 16)."""
    _fields_ = [
        ("a", C.c_void_p), ("w", C.c_void_p), ("w_scale", C.c_void_p), ("c", C.c_void_p), ("row_scale", C.c_void_p),
        ("sorted_token_idxes", C.c_void_p), ("expert_ids", C.c_void_p), ("n_padded_tokens", C.c_void_p),
        ("w_expert_stride", C.c_int64), ("w_scale_expert_stride", C.c_int64), ("n_flat", C.c_int64),
        ("K", C.c_int64), ("N", C.c_int64), ("lda", C.c_int64), ("ldw", C.c_int64), ("ldc", C.c_int64),
        ("a_div", C.c_int32), ("n_experts", C.c_int32), ("max_blocks", C.c_int32), ("dtype", C.c_int32),
        ("flags", C.c_int32),
    ]


class MoeMxfp4GemmArgs(C.Structure):
    """struct slm_moe_mxfp4_gemm_args (include/slm_hip.h section 21): slm_moe_fp8_gemm_args, field for field (w_scale:
    e8m0 bytes, its expert stride in bytes), plus the scales' row stride."""
    _fields_ = MoeFp8GemmArgs._fields_ + [("lds", C.c_int64)]


class MoeRouterArgs(C.Structure):
    """struct slm_moe_router_args (include/slm_hip.h section 17)."""
    _fields_ = [
        ("x", C.c_void_p), ("gate_w", C.c_void_p), ("correction_bias", C.c_void_p), ("weights", C.c_void_p),
        ("indices", C.c_void_p), ("logits_out", C.c_void_p), ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_int64), ("n_tokens", C.c_int64), ("hidden", C.c_int64),
        ("ldx", C.c_int64), ("ldw", C.c_int64),
        ("n_experts", C.c_int32), ("topk", C.c_int32), ("dtype", C.c_int32), ("scoring", C.c_int32),
        ("renormalize", C.c_int32), ("n_expert_groups", C.c_int32), ("topk_group", C.c_int32),
        ("scaling_factor", C.c_float),
    ]


SLM_ROUTER_SOFTMAX, SLM_ROUTER_GROUPED_SIGMOID = 0, 1   # slm_moe_router_args.scoring


class MlaArgs(C.Structure):
    """struct slm_mla_args (include/slm_hip.h section 11)."""
    _fields_ = [
        ("out", C.c_void_p), ("q", C.c_void_p), ("q_rope", C.c_void_p), ("kv_cache", C.c_void_p),
        ("k_rope_cache", C.c_void_p),
        ("o_stride", C.c_int64 * 2), ("q_stride", C.c_int64 * 2), ("q_rope_stride", C.c_int64 * 2),
        ("kv_stride", C.c_int64), ("k_rope_stride", C.c_int64),
        ("q_cu_lens", C.c_void_p), ("kv_cu_lens", C.c_void_p), ("block_table", C.c_void_p),
        ("block_cu_lens", C.c_void_p),
        ("dtype", C.c_int32), ("batch_size", C.c_int32), ("n_tokens", C.c_int32), ("n_heads", C.c_int32),
        ("head_dim", C.c_int32), ("rope_head_dim", C.c_int32), ("block_size", C.c_int32),
        ("max_q_len", C.c_int32), ("max_kv_len", C.c_int32), ("sm_scale", C.c_float),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("num_splits", C.c_int32), ("reserved", C.c_int32),
    ]


class GemmaNormArgs(C.Structure):
    """struct slm_gemma_norm_args (include/slm_hip.h section 12)."""
    _fields_ = [
        ("out", C.c_void_p), ("x", C.c_void_p), ("partials", C.c_void_p), ("post_weight", C.c_void_p),
        ("pre_weight", C.c_void_p), ("residual", C.c_void_p), ("table", C.c_void_p), ("token_ids", C.c_void_p),
        ("vocab", C.c_int64), ("n_tokens", C.c_int64), ("dim", C.c_int64),
        ("n_splits", C.c_int32), ("dtype", C.c_int32), ("x_scale", C.c_float), ("eps", C.c_float),
    ]


class LinearArgs(C.Structure):
    """struct slm_linear_args (include/slm_hip.h section 13)."""
    _fields_ = [
        ("a", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("c", C.c_void_p),
        ("M", C.c_int64), ("K", C.c_int64), ("N", C.c_int64),
        ("lda", C.c_int64), ("ldw", C.c_int64), ("ldc", C.c_int64),
        ("dtype", C.c_int32), ("flags", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class Fp8LinearArgs(C.Structure):
    """struct slm_fp8_linear_args (include/slm_hip.h section 15): slm_linear_args, field for field, plus w_scale."""
    _fields_ = LinearArgs._fields_ + [("w_scale", C.c_void_p)]


class Mxfp4LinearArgs(C.Structure):
    """struct slm_mxfp4_linear_args (include/slm_hip.h section 20): slm_linear_args, field for field, plus the e8m0
    block scales and their row stride."""
    _fields_ = LinearArgs._fields_ + [("w_scale", C.c_void_p), ("lds", C.c_int64)]


class LinearPlanInfo(C.Structure):
    """struct slm_linear_plan_info (include/slm_hip.h section 13)."""
    _fields_ = [
        ("row_tiles", C.c_int32), ("waves", C.c_int32), ("row_blocks", C.c_int32), ("col_groups", C.c_int32),
        ("split_k", C.c_int32), ("n_chunks", C.c_int32), ("tail_units", C.c_int32),
        ("slice_chunk", C.c_int32 * 17),
        ("lds_bytes", C.c_uint64), ("workspace_bytes", C.c_uint64),
    ]

    def slice_k_range(self, j: int):
        """[k0, k1) of K slice j: whole 128-deep chunks, the K % 128 tail with the last slice."""
        k0, k1 = 128 * self.slice_chunk[j], 128 * self.slice_chunk[j + 1]
        return k0, k1 + (32 * self.tail_units if j == self.split_k - 1 else 0)


SLM_LINEAR_DEFER_REDUCE = 1
SLM_LINEAR_SILU_MUL = 2
SLM_LINEAR_SHARES_CHIP = 4

SLM_MOE_SILU_MUL = 2    # slm_moe_gemm flags
SLM_MOE_GEMM_BLOCK = 32  # rows per block of the grouped GEMM: the align step's block_size


_lib = None


def lib() -> C.CDLL:
    """Load libslm_hip.so or raise -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SlmError(
            f"{LIB_PATH} not found: build it with `python -m scalellm_amd.build` "
            "(hipcc --offload-arch=gfx950). scalellm_amd has no CPU / PyTorch fallback.")
    # ONE HIP runtime per process: torch ships its own libamdhip64.so.7 (same SONAME as
    # /opt/rocm's).  Importing torch first makes libslm_hip.so bind to the runtime torch already
    # loaded -- the one that owns the device context, streams and allocations we are handed.
    # (Loaded the other way round, kernels launch on a second runtime that sees no device.)
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    L.slm_status_string.restype = C.c_char_p
    L.slm_status_string.argtypes = [C.c_int]
    L.slm_version.restype = C.c_char_p
    L.slm_last_hip_error.restype = C.c_char_p
    L.slm_paged_kv_varlen_mha.restype = C.c_int
    L.slm_paged_kv_varlen_mha.argtypes = [C.POINTER(AttnArgs), C.c_void_p]
    L.slm_paged_kv_varlen_mha_workspace_bytes.restype = C.c_size_t
    L.slm_paged_kv_varlen_mha_workspace_bytes.argtypes = [C.POINTER(AttnArgs)]
    L.slm_paged_kv_varlen_mha_auto_splits.restype = C.c_int32
    L.slm_paged_kv_varlen_mha_auto_splits.argtypes = [C.POINTER(AttnArgs)]
    L.slm_paged_kv_varlen_mha_decode_kernel.restype = C.c_int32
    L.slm_paged_kv_varlen_mha_decode_kernel.argtypes = [C.POINTER(AttnArgs)]
    L.slm_paged_kv_varlen_mha_kv_near.restype = C.c_int32
    L.slm_paged_kv_varlen_mha_kv_near.argtypes = [C.POINTER(AttnArgs)]
    L.slm_build_step_inputs.restype = C.c_int
    L.slm_build_step_inputs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
    L.slm_set_kv_cache.restype = C.c_int
    L.slm_set_kv_cache.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                   C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_void_p]
    for name, restype, argtypes in [
        ("slm_w4_packed_weight_bytes", C.c_size_t, [C.c_int64, C.c_int64]),
        ("slm_w4_packed_sz_bytes", C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
        ("slm_w4_prepack", C.c_int,
         [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
          C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
        ("slm_w4_prepack_weights", C.c_int,
         [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
        ("slm_w4_prepack_sz", C.c_int,
         [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
          C.c_void_p]),
        ("slm_w8_packed_rows", C.c_int64, [C.c_int64]),
        ("slm_w8_packed_group_size", C.c_int64, [C.c_int64, C.c_int64]),
        ("slm_w8_prepack_weights", C.c_int,
         [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
        ("slm_w8_prepack_sz", C.c_int,
         [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
          C.c_void_p]),
        ("slm_w4a16_gemm_workspace_bytes", C.c_size_t, [C.POINTER(W4GemmArgs)]),
        ("slm_w4a16_gemm", C.c_int, [C.POINTER(W4GemmArgs), C.c_void_p]),
        ("slm_w4a16_gemm_deferred_splits", C.c_int32, [C.POINTER(W4GemmArgs)]),
        ("slm_w4a16_gemm_plan", C.c_int, [C.POINTER(W4GemmArgs), C.POINTER(W4PlanInfo)]),
        ("slm_w4a16_gemv_norm_supported", C.c_int32, [C.POINTER(W4GemmArgs)]),
        ("slm_w4a16_gemv_norm", C.c_int, [C.POINTER(W4GemmArgs), C.POINTER(W4NormPrologue), C.c_void_p]),
        ("slm_rms_norm_splitk", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float,
          C.c_int32, C.c_void_p]),
        ("slm_w4_dequant", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
          C.c_void_p]),
        ("slm_rms_norm", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float,
          C.c_int32, C.c_void_p]),
        ("slm_rope_kv_append", C.c_int,
         [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
          C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
          C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
        ("slm_rope_kv_append_splitk", C.c_int,
         [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
          C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
          C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
        ("slm_silu_mul", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
        ("slm_layer_norm", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_int32, C.c_void_p]),
        ("slm_gelu", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
        ("slm_decode_advance", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
          C.c_void_p, C.c_void_p]),
        ("slm_tuning_set", C.c_int, [C.c_char_p, C.c_int32]),
        ("slm_tuning_clear", C.c_int, [C.c_char_p]),
        ("slm_tuning_get", C.c_int, [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        ("slm_shm_alloc", C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.c_int32]),
        ("slm_shm_free", C.c_int, [C.c_void_p]),
        ("slm_shm_export", C.c_int, [C.c_void_p, C.c_char_p]),
        ("slm_shm_import", C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
        ("slm_shm_close", C.c_int, [C.c_void_p]),
        ("slm_shm_enable_peer_access", C.c_int, [C.c_int32, C.c_int32]),
        ("slm_ar_signal_bytes", C.c_size_t, []),
        ("slm_ar_read_error", C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
        ("slm_allreduce", C.c_int, [C.POINTER(ArArgs), C.c_void_p]),
        ("slm_allreduce_simulate", C.c_int, [C.POINTER(ArArgs), C.c_int32, C.c_void_p]),
        ("slm_decode_lane_split", C.c_int32, [C.POINTER(LaneQuery)]),
        ("slm_decode_lane_policy_record", C.c_int, [C.POINTER(LaneQuery), C.c_float, C.c_float]),
        ("slm_decode_lane_policy_clear", C.c_int, []),
        ("slm_decode_lane_policy_measured", C.c_int32, [C.POINTER(LaneQuery)]),
        ("slm_sample_workspace_bytes", C.c_size_t, [C.POINTER(SamplingArgs)]),
        ("slm_sample", C.c_int, [C.POINTER(SamplingArgs), C.c_void_p]),
        ("slm_logits_process", C.c_int, [C.POINTER(SamplingArgs), C.c_void_p]),
        ("slm_rejection_sample_workspace_bytes", C.c_size_t, [C.POINTER(RejectionArgs)]),
        ("slm_rejection_sample", C.c_int, [C.POINTER(RejectionArgs), C.c_void_p]),
        ("slm_moe_topk_softmax", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
        ("slm_moe_grouped_topk_sigmoid", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
          C.c_float, C.c_void_p]),
        ("slm_moe_align_capacity", C.c_int,
         [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        ("slm_moe_align_block", C.c_int, [C.POINTER(MoeAlignArgs), C.c_void_p]),
        ("slm_moe_sum", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_void_p]),
        ("slm_moe_sum_add", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_void_p]),
        ("slm_mla_rope_append", C.c_int,
         [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int32,
          C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
          C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
        ("slm_mla_rope_append_splitk", C.c_int,
         [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int32,
          C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
          C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
        ("slm_qk_norm_rope_kv_append", C.c_int,
         [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float,
          C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
          C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
        ("slm_qk_norm_rope_kv_append_splitk", C.c_int,
         [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
          C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
          C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
        ("slm_moe_w4a16_gemm", C.c_int, [C.POINTER(MoeGemmArgs), C.c_void_p]),
        ("slm_moe_gemm", C.c_int, [C.POINTER(MoeDenseGemmArgs), C.c_void_p]),
        ("slm_mla_paged_kv_workspace_bytes", C.c_size_t, [C.POINTER(MlaArgs)]),
        ("slm_mla_paged_kv_auto_splits", C.c_int32, [C.POINTER(MlaArgs)]),
        ("slm_mla_paged_kv", C.c_int, [C.POINTER(MlaArgs), C.c_void_p]),
        ("slm_mla_set_kv_cache", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
          C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
        ("slm_gemma_norm", C.c_int, [C.POINTER(GemmaNormArgs), C.c_void_p]),
        ("slm_linear", C.c_int, [C.POINTER(LinearArgs), C.c_void_p]),
        ("slm_linear_workspace_bytes", C.c_size_t, [C.POINTER(LinearArgs)]),
        ("slm_linear_deferred_splits", C.c_int32, [C.POINTER(LinearArgs)]),
        ("slm_linear_plan", C.c_int, [C.POINTER(LinearArgs), C.POINTER(LinearPlanInfo)]),
        ("slm_fp8_linear", C.c_int, [C.POINTER(Fp8LinearArgs), C.c_void_p]),
        ("slm_fp8_linear_workspace_bytes", C.c_size_t, [C.POINTER(Fp8LinearArgs)]),
        ("slm_fp8_linear_deferred_splits", C.c_int32, [C.POINTER(Fp8LinearArgs)]),
        ("slm_fp8_linear_plan", C.c_int, [C.POINTER(Fp8LinearArgs), C.POINTER(LinearPlanInfo)]),
        ("slm_moe_fp8_gemm", C.c_int, [C.POINTER(MoeFp8GemmArgs), C.c_void_p]),
        ("slm_mxfp4_linear", C.c_int, [C.POINTER(Mxfp4LinearArgs), C.c_void_p]),
        ("slm_mxfp4_linear_deferred_splits", C.c_int32, [C.POINTER(Mxfp4LinearArgs)]),
        ("slm_mxfp4_linear_plan", C.c_int, [C.POINTER(Mxfp4LinearArgs), C.POINTER(LinearPlanInfo)]),
        ("slm_moe_mxfp4_gemm", C.c_int, [C.POINTER(MoeMxfp4GemmArgs), C.c_void_p]),
        ("slm_moe_router", C.c_int, [C.POINTER(MoeRouterArgs), C.c_void_p]),
        ("slm_moe_router_splits", C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int32)]),
        ("slm_moe_router_workspace_bytes", C.c_int,
         [C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_size_t)]),
        ("slm_soft_cap", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_int32, C.c_void_p]),
        ("slm_permute_index_map", C.c_int,
         [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
        ("slm_permute_mask_map", C.c_int,
         [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        ("slm_permute_rows", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
        ("slm_unpermute_rows", C.c_int,
         [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int64,
          C.c_int32, C.c_void_p]),
    ]:
        fn = getattr(L, name)  # AttributeError here = library/header mismatch: fail loudly
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    if rc != 0:
        detail = f" [{lib().slm_last_hip_error().decode()}]" if rc == -4 else ""
        raise SlmError(f"{what} failed: {lib().slm_status_string(rc).decode()} ({rc}){detail}")
