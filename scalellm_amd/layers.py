"""Host-side mirror of the reference's LAYER-level operator API for the hot path, built on
scalellm_amd.kernels (-> libslm_hip.so).  Same class / method names and argument meaning as
the reference so parity tests read like the reference's own layer tests.

  InputParameters      <- llm::InputParameters        src/models/parameters.h:11-56
  KVCache              <- llm::KVCache                src/memory/kv_cache.h:11-67
  HipAttnHandler       <- llm::ScaleAttnHandler       src/layers/attention/scale_attn_handler.cpp
                          (AttentionHandler interface src/layers/attention/handler.h:15-48)
  Attention            <- llm::AttentionImpl          src/layers/attention/attention.cpp:7-46
  ColumnParallelQLinear / RowParallelQLinear
                       <- {Column,Row}ParallelQLinear{AWQ,GPTQ}MarlinImpl
                          src/layers/quantization/qlinear_awq_marlin_impl.cpp:128-366,
                          qlinear_gptq_marlin_impl.cpp:74-330 (TP sharding dims, lazy repack on
                          first forward, all-reduce then bias for row-parallel)
  ColumnParallelLinear / RowParallelLinear
                       <- {Column,Row}ParallelLinearImpl  src/layers/linear/parallel_linear.cpp:221-308
                          (unquantised f16 / bf16 weights [out, in] in checkpoint layout -> slm_linear)
  LayerNorm            <- llm::LayerNormImpl          src/layers/normalization.h:68-110
  GemmaRMSNorm         <- llm::GemmaRMSNormImpl       src/layers/normalization.h:142-168
  Activation           <- llm::Activation             src/layers/activation.h:36-46, activation.cpp:80-140
                          (the LayerNorm model families -- GPT-2, BASELINE configs[0] -- next to the
                          RMSNorm / SiLU pair the Llama path uses)
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import kernels
from .model_parallel import (ParallelArgs, gather_from_model_parallel_region,
                             reduce_from_model_parallel_region)


@dataclass
class InputParameters:
    """models/parameters.h:11-56 (the attention-relevant fields)."""
    q_cu_seq_lens: torch.Tensor       # [batch + 1] int32
    kv_cu_seq_lens: torch.Tensor      # [batch + 1] int32
    new_cache_slots: torch.Tensor     # [n_tokens] int32
    block_tables: torch.Tensor        # flattened first-slot ids
    cu_block_lens: torch.Tensor       # [batch + 1] int32
    q_max_seq_len: int = 0
    kv_max_seq_len: int = 0
    # extension (not in models/parameters.h): cu_seq_lens.back() as Batch::prepare_model_input has it on
    # the host (batch.cpp:137).  A scheduling hint like the two maxima above: lets the attention plan recognise
    # a uniform batch (kernels.paged_kv_varlen_mha, total_kv_len).  0 = unknown: derived from the host-known
    # SIZES where they settle it (uniform_kv_hint below -- what an unchanged engine gets); < 0 = known NOT to
    # be uniform (no derivation: a graph captured over padded static buffers, the half of a ragged batch)
    kv_total_len: int = 0


def uniform_kv_hint(kv_total_len: int, n_seqs: int, q_max_seq_len: int, kv_max_seq_len: int,
                    block_table_len: int, block_size: int) -> int:
    """The total_kv_len the attention plan is given (slm_attn_args::total_kv_len), from what the HOST knows.

    The caller's own value wins (> 0; < 0 means "not uniform": 0 is returned).  Unknown (0): the reference's
    InputParameters (models/parameters.h:11-56) carries the two maxima and the flattened block table
    (batch.cpp:206-209), whose LENGTH the host has: a pure-decode batch whose table holds exactly
    n_seqs * ceil(kv_max_seq_len / block_size) entries has, in EVERY sequence, more than kv_max_seq_len -
    block_size tokens -- as uniform as the plan needs (one workgroup per sequence and head group is then the
    balanced partition already) -- and is reported as n_seqs * kv_max_seq_len.  Anything else: 0 (the balanced
    partition, right for every batch).  Like every hint of the call it only shapes the launch."""
    if kv_total_len > 0:
        return int(kv_total_len)
    if kv_total_len < 0 or n_seqs <= 0 or q_max_seq_len > 1 or kv_max_seq_len <= 0 or block_size <= 0:
        return 0
    blocks = (kv_max_seq_len + block_size - 1) // block_size
    return n_seqs * kv_max_seq_len if block_table_len == n_seqs * blocks else 0


class KVCache:
    """[n_blocks * block_size, n_kv_heads, head_dim] K and V tensors (memory/kv_cache.cpp:15-27)."""

    def __init__(self, n_blocks: int, block_size: int, n_kv_heads: int, head_dim: int,
                 dtype: torch.dtype, device):
        self._block_size = block_size
        self.key_cache = torch.empty(n_blocks * block_size, n_kv_heads, head_dim, dtype=dtype,
                                     device=device)
        self.value_cache = torch.empty_like(self.key_cache)

    def block_size(self) -> int:
        return self._block_size

    def get_kv_cache(self) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.key_cache, self.value_cache

    def set_kv_cache(self, slot_ids: torch.Tensor, keys: torch.Tensor, values: torch.Tensor) -> None:
        kernels.set_kv_cache(slot_ids, keys, values, self.key_cache, self.value_cache)


class HipAttnHandler:
    """AttentionHandler over the HIP kernels (handler.h:15-48).  RoPE and the KV append are one
    fused launch: apply_pos_emb() only records its inputs and append_kv_cache() issues the fused
    kernel (the reference always calls them back to back: attention.cpp:36-39)."""

    def __init__(self, sm_scale: float, logits_soft_cap: float = 0.0,
                 alibi_slopes: Optional[torch.Tensor] = None, rotary_dim: int = 0,
                 cos_sin: Optional[torch.Tensor] = None, interleaved: bool = False,
                 q_norm: Optional[torch.Tensor] = None, k_norm: Optional[torch.Tensor] = None,
                 qk_norm_eps: Optional[float] = None):
        self.sm_scale = sm_scale
        self.logits_soft_cap = logits_soft_cap
        self.alibi_slopes = alibi_slopes
        self.rotary_dim, self.cos_sin, self.interleaved = rotary_dim, cos_sin, interleaved
        self._pending = None
        # fp32 split-K slabs of the fused qkv GEMM (kernels.DeferredPartials), consumed by the next
        # append_kv_cache(): the RoPE + append kernel then also does the split-K reduction
        self.qkv_partials = None
        # Qwen3's per-head RMSNorm of q and k ([head_dim] weights) before RoPE: append_kv_cache() then issues
        # kernels.qk_norm_rope_kv_append.  qk_norm_fused = False runs the composition of the older entry points
        # instead (copies, two rms_norm, apply_rotary_pos_emb), which takes no deferred slabs
        if (q_norm is None) != (k_norm is None) or (q_norm is not None and qk_norm_eps is None):
            raise kernels.SlmError("q_norm and k_norm come together, with qk_norm_eps")
        if q_norm is not None and cos_sin is None:
            raise kernels.SlmError("the QK-norm prologue needs RoPE (cos_sin)")
        self.q_norm, self.k_norm, self.qk_norm_eps = q_norm, k_norm, qk_norm_eps
        self.qk_norm_fused = True

    @staticmethod
    def build_cos_sin(rotary_dim: int, max_position: int, inv_freq: torch.Tensor) -> torch.Tensor:
        """[max_position, rotary_dim] = cos | sin, fp32 (RotaryEmbeddingKernel pos_embedding.cpp
        :183-197 builds the same table in the activation dtype; fp32 keeps RoPE exact)."""
        t = torch.arange(max_position, dtype=torch.float32, device=inv_freq.device)
        freqs = torch.einsum("i,j->ij", t, inv_freq.float())
        return torch.cat([freqs.cos(), freqs.sin()], dim=-1).contiguous()

    def apply_pos_emb(self, query, key, positions):
        if self.cos_sin is not None and positions is not None:
            self._pending = positions
        return query, key

    def append_kv_cache(self, kv_cache: KVCache, query, key, value, input_params: InputParameters):
        kc, vc = kv_cache.get_kv_cache()
        partials, self.qkv_partials = self.qkv_partials, None
        if self.q_norm is not None:
            if self._pending is None:
                raise kernels.SlmError("the QK-norm prologue needs positions")
            positions, self._pending = self._pending, None
            if self.qk_norm_fused:
                kernels.qk_norm_rope_kv_append(query, key, value, self.q_norm, self.k_norm, self.qk_norm_eps,
                                               positions, self.cos_sin, self.interleaved,
                                               slot_ids=input_params.new_cache_slots, key_cache=kc, value_cache=vc,
                                               partials=partials)
                return
            if partials:
                raise kernels.SlmError("the unfused QK-norm composition takes no deferred qkv partials")
            for x, w in ((query, self.q_norm), (key, self.k_norm)):
                rows = x.reshape(-1, x.size(-1)).contiguous()  # a copy: x is a column slice of the qkv row
                kernels.rms_norm(rows, rows, w, self.qk_norm_eps)
                x.copy_(rows.view_as(x))
            kernels.apply_rotary_pos_emb(query, key, positions, self.cos_sin, self.rotary_dim, self.interleaved,
                                         value=value, slot_ids=input_params.new_cache_slots, key_cache=kc,
                                         value_cache=vc)
            return
        if self._pending is not None:
            kernels.apply_rotary_pos_emb(query, key, self._pending, self.cos_sin, self.rotary_dim,
                                         self.interleaved, value=value,
                                         slot_ids=input_params.new_cache_slots, key_cache=kc,
                                         value_cache=vc, partials=partials)
            self._pending = None
        else:
            if partials:
                raise kernels.SlmError("deferred qkv partials need the rotary path (no RoPE configured)")
            kernels.set_kv_cache(input_params.new_cache_slots, key, value, kc, vc)

    def batch_decode(self, query, kv_cache: KVCache, input_params: InputParameters,
                     sliding_window: int, output: torch.Tensor, phase: int = 0) -> None:
        kc, vc = kv_cache.get_kv_cache()
        total = getattr(input_params, "kv_total_len", 0)
        if total == 0 and not torch.cuda.is_current_stream_capturing():
            # (an unchanged engine fills no hint: the sizes it hands over settle the uniform case.  Not under
            # capture: a captured call sees padded static buffers and bounds, not a batch)
            total = uniform_kv_hint(0, input_params.q_cu_seq_lens.numel() - 1, input_params.q_max_seq_len,
                                    input_params.kv_max_seq_len, input_params.block_tables.numel(),
                                    kv_cache.block_size())
        kernels.paged_kv_varlen_mha(output, query, kc, vc, input_params.q_cu_seq_lens,
                                    input_params.kv_cu_seq_lens, input_params.block_tables,
                                    input_params.cu_block_lens, self.alibi_slopes,
                                    kv_cache.block_size(), input_params.q_max_seq_len,
                                    kernels.visible_kv_hint(input_params.kv_max_seq_len, input_params.q_max_seq_len,
                                                            sliding_window), self.sm_scale,
                                    self.logits_soft_cap, sliding_window,
                                    total_kv_len=total, phase=phase)


class Attention:
    """AttentionImpl::forward (attention.cpp:22-46): rope -> append -> paged attention."""

    def __init__(self, n_heads: int, n_kv_heads: int, head_dim: int, handler: HipAttnHandler,
                 sliding_window: int = -1):
        self.n_heads, self.n_kv_heads, self.head_dim = n_heads, n_kv_heads, head_dim
        self.handler, self.sliding_window = handler, sliding_window

    def append(self, query, key, value, positions, kv_cache: KVCache, input_params: InputParameters,
               qkv_partials=None):
        """First half of forward(): RoPE + KV append (attention.cpp:36-39).  Returns the [T, H, D] view
        of the (rotated) query for decode()."""
        self.handler.qkv_partials = qkv_partials if qkv_partials else None
        T = query.size(0)
        q = query.view(T, self.n_heads, self.head_dim)
        k = key.view(T, self.n_kv_heads, self.head_dim)
        v = value.view(T, self.n_kv_heads, self.head_dim)
        q, k = self.handler.apply_pos_emb(q, k, positions)
        self.handler.append_kv_cache(kv_cache, q, k, v, input_params)
        return q

    def decode(self, q, kv_cache: KVCache, input_params: InputParameters,
               output: Optional[torch.Tensor] = None, phase: int = 0):
        """Second half of forward(): the paged attention itself (attention.cpp:41-42)."""
        T = q.size(0)
        if output is None:
            output = torch.empty(T, self.n_heads, self.head_dim, dtype=q.dtype, device=q.device)
        self.handler.batch_decode(q, kv_cache, input_params, self.sliding_window, output, phase=phase)
        return output.view(T, self.n_heads * self.head_dim)

    def forward(self, query, key, value, positions, kv_cache: KVCache,
                input_params: InputParameters, output: Optional[torch.Tensor] = None,
                qkv_partials=None):
        """qkv_partials (truthy kernels.DeferredPartials): query / key / value are the column slices
        of a fused qkv GEMM output that was left as split-K slabs (ColumnParallelQLinear.forward(
        defer_splitk=True)); the RoPE + append kernel sums them."""
        q = self.append(query, key, value, positions, kv_cache, input_params, qkv_partials)
        return self.decode(q, kv_cache, input_params, output)


# ---------------------------------------------------------------------------------------
# int4 linear layers
# ---------------------------------------------------------------------------------------
@dataclass
class QuantArgs:
    """layers/quantization/quant_args.h:10-33.  quant_method "fp8" with bits = 8 selects e4m3 weight-only (W8A16)
    weights where a layer offers them (moe.FusedMoE / ExpertParallelMoE; LlamaDecodeStep takes quant_method="fp8"
    directly); group_size, desc_act and zero_point mean nothing there and are ignored.  quant_method "mxfp4" is OCP
    MXFP4 weight-only (W4A16: e2m1 nibbles, one e8m0 scale byte per 32 k, bits = 4 and group_size = 32 by the format):
    LlamaDecodeStep takes quant_method="mxfp4" directly (layers.{Column,Row}ParallelMxfp4Linear), and
    QuantArgs("mxfp4", 4) selects moe.MoEMxfp4Experts in moe.FusedMoE / ExpertParallelMoE (the other fields ignored)."""
    quant_method: str = "awq"   # "awq" | "gptq" | "fp8" | "mxfp4"
    bits: int = 4
    group_size: int = 128
    desc_act: bool = False
    zero_point: bool = True


class _QLinearBase:
    def __init__(self, in_features: int, out_features: int, bias: bool, quant_args: QuantArgs,
                 parallel_args: ParallelArgs, dtype: torch.dtype, device):
        if quant_args.bits not in (4, 8):  # qlinear_awq_marlin_impl.cpp:25-26: 4 and 8
            raise kernels.SlmError(f"only 4- and 8-bit weights are supported, got bits = {quant_args.bits}")
        self.in_features, self.out_features = in_features, out_features
        self.quant_args, self.parallel_args = quant_args, parallel_args
        self.dtype, self.device = dtype, device
        self.has_bias = bias
        self.bias: Optional[torch.Tensor] = None
        self._ckpt: Dict[str, torch.Tensor] = {}
        self._packed: Optional[kernels.PackedW4] = None
        self.paired = False  # merged [gate | up] weight packed for the fused SiLU*mul epilogue

    # checkpoint-format tensors for THIS rank's shard
    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        for name in ("qweight", "qzeros", "scales", "g_idx", "bias"):
            if name in sd:
                self._ckpt[name] = sd[name].to(self.device)
        self._packed = None

    def verify_loaded_weights(self) -> None:
        for name in ("qweight", "qzeros", "scales"):
            assert name in self._ckpt, f"{name} is not loaded"
        assert (not self.has_bias) or "bias" in self._ckpt, "bias is not loaded"

    def _repack(self) -> None:  # lazily on first forward, like the reference (inside warm-up)
        c = self._ckpt
        scales = c["scales"].to(self.dtype).contiguous()
        if self.quant_args.quant_method == "awq":
            self._packed = kernels.awq_repack(c["qweight"], c["qzeros"], scales,
                                              self.quant_args.group_size, paired=self.paired,
                                              bits=self.quant_args.bits)
        else:
            self._packed = kernels.gptq_repack(c["qweight"], c["qzeros"], scales,
                                               self.quant_args.group_size, c.get("g_idx"),
                                               paired=self.paired, bits=self.quant_args.bits)
        if self.has_bias:
            self.bias = c["bias"].to(self.dtype).contiguous()
            if self.paired:  # the bias follows the packed column order: gate / up 32-column tiles alternate
                n = self.bias.numel()
                self.bias = torch.stack([self.bias[:n // 2].view(-1, 32), self.bias[n // 2:].view(-1, 32)],
                                        dim=1).reshape(-1).contiguous()
        self._ckpt = {}

    def _gemm(self, x: torch.Tensor, bias: Optional[torch.Tensor],
              out: Optional[torch.Tensor], defer_splitk: bool = False,
              norm: Optional[kernels.NormPrologue] = None) -> torch.Tensor:
        if self._packed is None:
            self._repack()
        x2 = x.reshape(-1, x.size(-1))
        if self.paired:
            if out is None:
                out = torch.empty(x2.size(0), self._packed.N // 2, dtype=x.dtype, device=x.device)
            kernels.gptq_gemm(x2, self._packed, out, bias, silu_mul=True, norm=norm)
            self.deferred, self.deferred_splits = kernels.DeferredPartials(), 0
            return out
        if out is None:
            out = torch.empty(x2.size(0), self._packed.N, dtype=x.dtype, device=x.device)
        # truthy: `out` was NOT written, fp32 split-K slabs wait in the deferred buffer for
        # kernels.rms_norm(..., partials=handle) (kernels.gptq_gemm, defer_reduce)
        self.deferred = kernels.gptq_gemm(x2, self._packed, out, bias, defer_reduce=defer_splitk,
                                          norm=norm)
        self.deferred_splits = int(self.deferred)
        return out


class ColumnParallelQLinear(_QLinearBase):
    """Y = X W + b with W sharded along N (qlinear_awq_marlin_impl.cpp:128-254).
    in_features / out_features are the FULL sizes; this rank holds out_features / world_size."""

    def __init__(self, in_features, out_features, bias, quant_args, gather_output,
                 parallel_args, dtype, device, act_mul: Optional[str] = None):
        """act_mul="silu": the weight is the MLP's merged [gate | up] projection
        (multi_parallel_linear.cpp:14-41) and forward returns act_and_mul of it,
        silu(gate) * up of width out_features / 2 per rank (activation_kernels.cu:84), computed in
        the GEMM epilogue -- bit-identical to forward + kernels.silu_and_mul, one launch less."""
        super().__init__(in_features, out_features, bias, quant_args, parallel_args, dtype, device)
        self.gather_output = gather_output
        if act_mul not in (None, "silu"):
            raise ValueError(f"unsupported fused activation {act_mul!r}")
        self.paired = act_mul == "silu"
        if self.paired and gather_output:
            raise ValueError("act_mul needs the sharded output (gather_output=False)")

    def _defers(self, defer_splitk: bool) -> bool:
        return defer_splitk and not self.has_bias and not self.paired and \
            not (self.parallel_args.world_size > 1 and self.gather_output)

    def norm_supported(self, n_tokens: int, defer_splitk: bool = False) -> bool:
        """Can forward(..., norm=...) fold the preceding RMSNorm into this projection (M <= 4 GEMV)?"""
        if self._packed is None:
            self._repack()
        return kernels.gemv_norm_supported(n_tokens, self._packed, self.dtype, silu_mul=self.paired,
                                           defer_reduce=self._defers(defer_splitk))

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None,
                defer_splitk: bool = False,
                norm: Optional[kernels.NormPrologue] = None) -> torch.Tensor:
        """defer_splitk (no bias, no gather, not act_mul): a split-K GEMM leaves its fp32 slabs for
        the consumer (self.deferred is truthy then and `out` is NOT written) -- the fused qkv
        projection hands them to the RoPE + append kernel (Attention.forward(qkv_partials=...)).

        norm: `x` is the input of the RMSNorm that precedes this projection (input_layernorm_ /
        post_attention_layernorm_, models/meta/llama.h:174-176), which then runs in the GEMV's
        prologue (kernels.NormPrologue; only when norm_supported())."""
        if self._packed is None:
            self._repack()
        defer = self._defers(defer_splitk)
        y = self._gemm(x, self.bias if self.has_bias else None, out, defer_splitk=defer, norm=norm)
        if self.parallel_args.world_size > 1 and self.gather_output:
            y = gather_from_model_parallel_region(y, self.parallel_args)
        return y


class RowParallelQLinear(_QLinearBase):
    """Y = sum_ranks X_r W_r + b with W sharded along K (qlinear_awq_marlin_impl.cpp:257-366):
    GEMM, all-reduce, THEN bias (:357-363)."""

    def __init__(self, in_features, out_features, bias, quant_args, input_is_parallelized,
                 parallel_args, dtype, device):
        super().__init__(in_features, out_features, bias, quant_args, parallel_args, dtype, device)
        self.input_is_parallelized = input_is_parallelized

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None,
                reduce: bool = True, defer_splitk: bool = False) -> torch.Tensor:
        """reduce=False returns this rank's PARTIAL sums (no all-reduce, no bias): the caller owns
        the reduction (custom_allreduce.XgmiAllReduce fuses it with the residual add + RMSNorm).
        defer_splitk (single rank, no bias): a split-K GEMM leaves its fp32 slabs for the RMSNorm
        that follows (self.deferred is truthy then, and the returned tensor is NOT written)."""
        if self._packed is None:
            self._repack()
        if not self.input_is_parallelized and self.parallel_args.world_size > 1:
            from .model_parallel import scatter_to_model_parallel_region
            x = scatter_to_model_parallel_region(x, self.parallel_args).contiguous()
        if self.parallel_args.world_size > 1:
            y = self._gemm(x, None, out)
            if not reduce:
                if self.has_bias:
                    raise ValueError("reduce=False: the bias must be added after the reduction")
                return y
            reduce_from_model_parallel_region(y, self.parallel_args)
            if self.has_bias:
                y.add_(self.bias)
            return y
        return self._gemm(x, self.bias if self.has_bias else None, out,
                          defer_splitk=defer_splitk and not self.has_bias)


# ---------------------------------------------------------------------------------------
# unquantised f16 / bf16 linear layers
# ---------------------------------------------------------------------------------------
class _LinearBase:
    """What {Column,Row}ParallelLinearImpl share (parallel_linear.cpp:221-308): `weight` is this rank's
    shard of the checkpoint tensor [out, in], kept in checkpoint layout and streamed as it is by
    kernels.linear (slm_linear) -- nothing is repacked.  load_state_dict takes FULL checkpoint tensors
    and keeps this rank's chunk (StateDict::get_sharded_tensor, weight_utils.h:60-66); tensors that a
    dict does not hold are skipped (a checkpoint is spread over files and every file is offered to
    every layer), a tensor that arrives twice is refused."""

    def __init__(self, in_features: int, out_features: int, bias: bool, parallel_args: ParallelArgs,
                 dtype: torch.dtype, device):
        if dtype not in (torch.float16, torch.bfloat16):
            raise kernels.SlmError(f"unsupported dtype {dtype}: fp16 / bf16 only")
        self.in_features, self.out_features = in_features, out_features
        self.parallel_args, self.dtype, self.device = parallel_args, dtype, device
        self.has_bias = bias
        self.weight: Optional[torch.Tensor] = None
        self.bias: Optional[torch.Tensor] = None
        self._parts: Dict[str, list] = {}
        self.paired = False  # merged [gate | up] weight with the fused SiLU*mul epilogue
        self.deferred, self.deferred_splits = kernels.DeferredPartials(), 0

    def _shard(self, t: torch.Tensor, dim: int, what: str) -> torch.Tensor:
        pa = self.parallel_args
        if dim < 0 or pa.world_size <= 1:
            return t
        if t.size(dim) % pa.world_size:
            raise ValueError(f"can't divide {what} evenly on dim {dim} with world_size {pa.world_size}")
        return t.chunk(pa.world_size, dim)[pa.rank]

    def _set(self, name: str, t: torch.Tensor) -> None:
        want = (self.local_out, self.local_in) if name == "weight" else (self.local_out,)
        if tuple(t.shape) != want:
            raise ValueError(f"{name} size mismatch: {tuple(t.shape)} vs {want}")
        setattr(self, name, t.to(device=self.device, dtype=self.dtype).contiguous())

    def _load_one(self, sd: Dict[str, torch.Tensor], name: str, dim: int) -> None:
        if name not in sd:
            return
        if getattr(self, name) is not None:
            raise RuntimeError(f"{name} is loaded twice")
        self._set(name, self._shard(sd[name], dim, name))

    def _load_fused(self, sd: Dict[str, torch.Tensor], prefixes, name: str) -> None:
        """WeightUtils::load_fused_weight (weight_utils.h:48-58): one shard per prefix, kept until all
        prefixes have arrived, then concatenated on dim 0 (q | k | v, gate | up)."""
        parts = self._parts.setdefault(name, [None] * len(prefixes))
        for i, p in enumerate(prefixes):
            if p + name not in sd:
                continue
            if parts[i] is not None or getattr(self, name) is not None:
                raise RuntimeError(f"{p + name} is loaded twice")
            parts[i] = self._shard(sd[p + name], 0, p + name).to(self.device)
        if all(t is not None for t in parts):
            self._set(name, torch.cat(parts, dim=0))
            del self._parts[name]

    def load_shard(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> None:
        """THIS rank's shard, already cut (decode.LlamaDecodeStep shards its synthetic checkpoint itself:
        replicated KV heads are no equal chunks)."""
        for name, t in (("weight", weight), ("bias", bias)):
            if t is None:
                continue
            if getattr(self, name) is not None:
                raise RuntimeError(f"{name} is loaded twice")
            self._set(name, t)

    def verify_loaded_weights(self, prefix: str = "") -> None:
        if self.weight is None:
            raise RuntimeError(f"weight is not loaded for {prefix}weight")
        if self.has_bias and self.bias is None:
            raise RuntimeError(f"bias is not loaded for {prefix}bias")

    def _repack(self) -> None:
        """Nothing to do: the checkpoint layout IS the kernel's (kept for the call surface of the Q classes)."""

    def norm_supported(self, n_tokens: int, defer_splitk: bool = False) -> bool:
        return False  # no norm-prologue GEMV over dense weights

    def _linear(self, x: torch.Tensor, bias: Optional[torch.Tensor], out: Optional[torch.Tensor],
                defer_splitk: bool = False) -> torch.Tensor:
        self.verify_loaded_weights()
        x2 = x.reshape(-1, x.size(-1))
        n_out = self.local_out // 2 if self.paired else self.local_out
        if out is None:
            out = torch.empty(x2.size(0), n_out, dtype=x.dtype, device=x.device)
        # truthy: `out` was NOT written, fp32 split-K slabs wait in the deferred buffer for the consumer
        self.deferred = kernels.linear(x2, self.weight, out, bias, defer_reduce=defer_splitk and not self.paired,
                                       silu_mul=self.paired)
        self.deferred_splits = int(self.deferred)
        return out


class ColumnParallelLinear(_LinearBase):
    """ColumnParallelLinearImpl (parallel_linear.cpp:221-263): Y = X W^T + b, W [out, in] sharded on dim 0
    (bias on dim 0).  in_features / out_features are the FULL sizes; this rank holds out_features /
    world_size rows.  act_mul="silu": the weight is the MLP's merged [gate | up] projection
    (load_state_dict(sd, prefixes=["gate_proj.", "up_proj."])) and forward returns silu(gate) * up of
    width out_features / 2 per rank from the GEMM epilogue -- the bits of forward + kernels.silu_and_mul."""

    def __init__(self, in_features, out_features, bias, gather_output, parallel_args, dtype, device,
                 act_mul: Optional[str] = None):
        super().__init__(in_features, out_features, bias, parallel_args, dtype, device)
        if out_features % parallel_args.world_size:
            raise ValueError(f"out_features {out_features} not divisible by world_size {parallel_args.world_size}")
        self.local_in, self.local_out = in_features, out_features // parallel_args.world_size
        self.gather_output = gather_output
        if act_mul not in (None, "silu"):
            raise ValueError(f"unsupported fused activation {act_mul!r}")
        self.paired = act_mul == "silu"
        if self.paired and gather_output:
            raise ValueError("act_mul needs the sharded output (gather_output=False)")

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefixes=None) -> None:
        if prefixes:
            self._load_fused(sd, prefixes, "weight")
            if self.has_bias:
                self._load_fused(sd, prefixes, "bias")
            return
        self._load_one(sd, "weight", 0)
        if self.has_bias:
            self._load_one(sd, "bias", 0)

    def _defers(self, defer_splitk: bool) -> bool:
        return defer_splitk and not self.has_bias and not self.paired and \
            not (self.parallel_args.world_size > 1 and self.gather_output)

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, reduce: bool = True,
                defer_splitk: bool = False) -> torch.Tensor:
        """defer_splitk (no bias, no gather, not act_mul): a split-K call leaves its fp32 slabs for the
        consumer (self.deferred is truthy then and `out` is NOT written).  `reduce` is accepted for the
        common call surface; a column-parallel linear has no reduction."""
        y = self._linear(x, self.bias if self.has_bias else None, out, defer_splitk=self._defers(defer_splitk))
        if self.parallel_args.world_size > 1 and self.gather_output:
            y = gather_from_model_parallel_region(y, self.parallel_args)
        return y


class RowParallelLinear(_LinearBase):
    """RowParallelLinearImpl (parallel_linear.cpp:266-308): Y = sum_ranks X_r W_r^T + b, W [out, in] sharded
    on dim 1, the bias whole: GEMM, all-reduce, THEN bias (:299-306)."""

    def __init__(self, in_features, out_features, bias, input_is_parallelized, parallel_args, dtype, device):
        super().__init__(in_features, out_features, bias, parallel_args, dtype, device)
        if in_features % parallel_args.world_size:
            raise ValueError(f"in_features {in_features} not divisible by world_size {parallel_args.world_size}")
        self.local_in, self.local_out = in_features // parallel_args.world_size, out_features
        self.input_is_parallelized = input_is_parallelized

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefixes=None) -> None:
        if prefixes:
            raise ValueError("row-parallel linears are never fused (parallel_linear.h:28-33)")
        self._load_one(sd, "weight", 1)
        if self.has_bias:
            self._load_one(sd, "bias", -1)  # added once, after the reduction

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, reduce: bool = True,
                defer_splitk: bool = False) -> torch.Tensor:
        """reduce=False returns this rank's PARTIAL sums (no all-reduce, no bias): the caller owns the
        reduction.  defer_splitk (single rank, no bias): a split-K call leaves its fp32 slabs for the
        RMSNorm that follows (self.deferred is truthy then, and the returned tensor is NOT written)."""
        if not self.input_is_parallelized and self.parallel_args.world_size > 1:
            from .model_parallel import scatter_to_model_parallel_region
            x = scatter_to_model_parallel_region(x, self.parallel_args).contiguous()
        if self.parallel_args.world_size > 1:
            y = self._linear(x, None, out)
            if not reduce:
                if self.has_bias:
                    raise ValueError("reduce=False: the bias must be added after the reduction")
                return y
            reduce_from_model_parallel_region(y, self.parallel_args)
            if self.has_bias:
                y.add_(self.bias)
            return y
        return self._linear(x, self.bias if self.has_bias else None, out,
                            defer_splitk=defer_splitk and not self.has_bias)


# ---------------------------------------------------------------------------------------
# fp8 (e4m3) weight-only linear layers: W8A16 over slm_fp8_linear
# ---------------------------------------------------------------------------------------
class _Fp8LinearMixin:
    """What the two fp8 classes add to _LinearBase: `weight` is the checkpoint's float8_e4m3fn tensor, kept as bytes
    and never converted (kernels.fp8_linear streams it as it is); `weight_scale` arrives 0-d, [1], [N] or [N, 1]
    in any float dtype and is kept as fp32 [local_out], one scale per output channel (a per-tensor scale is
    expanded, in a fused load per shard).  An `input_scale` key is ignored: activations stay f16 / bf16.  A weight
    of any other dtype is an error -- quantising is the checkpoint's job (kernels.quantize_fp8_weight), not a
    side effect of loading."""

    weight_scale: Optional[torch.Tensor] = None

    def _set(self, name: str, t: torch.Tensor) -> None:
        if name == "weight":
            if t.dtype != torch.float8_e4m3fn:
                raise TypeError(f"fp8 linear: weight must be float8_e4m3fn, not {t.dtype} (quantize_fp8_weight "
                                "makes one; nothing is quantised on load)")
            if tuple(t.shape) != (self.local_out, self.local_in):
                raise ValueError(f"weight size mismatch: {tuple(t.shape)} vs {(self.local_out, self.local_in)}")
            self.weight = t.to(self.device).contiguous()
        elif name == "weight_scale":
            if tuple(t.shape) != (self.local_out,):
                raise ValueError(f"weight_scale size mismatch: {tuple(t.shape)} vs {(self.local_out,)}")
            self.weight_scale = t.to(device=self.device, dtype=torch.float32).contiguous()
        else:
            super()._set(name, t)

    @staticmethod
    def _channel_scale(t: torch.Tensor, rows: int, what: str) -> torch.Tensor:
        """0-d / [1] (per tensor) or [rows] / [rows, 1] (per channel) -> fp32 [rows]"""
        if not t.is_floating_point():
            raise TypeError(f"{what} must be a float tensor, not {t.dtype}")
        flat = t.reshape(-1).to(torch.float32)
        if flat.numel() == 1:
            return flat.expand(rows)
        if flat.numel() != rows or t.dim() > 2 or (t.dim() == 2 and t.size(1) != 1):
            raise ValueError(f"{what} size mismatch: {tuple(t.shape)} for {rows} output channels")
        return flat

    def _load_scale(self, sd: Dict[str, torch.Tensor], full_rows: int, dim: int) -> None:
        if "weight_scale" not in sd:
            return
        if self.weight_scale is not None:
            raise RuntimeError("weight_scale is loaded twice")
        full = self._channel_scale(sd["weight_scale"], full_rows, "weight_scale")
        self._set("weight_scale", self._shard(full, dim, "weight_scale"))

    def load_shard(self, weight: torch.Tensor, weight_scale: torch.Tensor,  # noqa: D401
                   bias: Optional[torch.Tensor] = None) -> None:
        """THIS rank's shard, already cut: float8_e4m3fn weight [local_out, local_in] and its scale
        (per tensor or [local_out])."""
        if self.weight_scale is not None:
            raise RuntimeError("weight_scale is loaded twice")
        super().load_shard(weight, bias)
        self._set("weight_scale", self._channel_scale(weight_scale, self.local_out, "weight_scale"))

    def verify_loaded_weights(self, prefix: str = "") -> None:
        super().verify_loaded_weights(prefix)
        if self.weight_scale is None:
            raise RuntimeError(f"weight_scale is not loaded for {prefix}weight_scale")

    def _linear(self, x: torch.Tensor, bias: Optional[torch.Tensor], out: Optional[torch.Tensor],
                defer_splitk: bool = False) -> torch.Tensor:
        self.verify_loaded_weights()
        x2 = x.reshape(-1, x.size(-1))
        n_out = self.local_out // 2 if self.paired else self.local_out
        if out is None:
            out = torch.empty(x2.size(0), n_out, dtype=x.dtype, device=x.device)
        self.deferred = kernels.fp8_linear(x2, self.weight, self.weight_scale, out, bias,
                                           defer_reduce=defer_splitk and not self.paired, silu_mul=self.paired)
        self.deferred_splits = int(self.deferred)
        return out


class ColumnParallelFp8Linear(_Fp8LinearMixin, ColumnParallelLinear):
    """ColumnParallelLinear over an fp8 checkpoint: weight AND weight_scale are sharded on dim 0.  A fused load
    (prefixes=[...]) concatenates the shards and expands each shard's own scale over its rows, so q | k | v and
    gate | up keep their per-tensor scales."""

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefixes=None) -> None:
        if not prefixes:
            self._load_one(sd, "weight", 0)
            self._load_scale(sd, self.out_features, 0)
            if self.has_bias:
                self._load_one(sd, "bias", 0)
            return
        # per prefix: (weight shard as bytes, scale over the shard's rows); both tensors of a prefix come together
        parts = self._parts.setdefault("weight", [None] * len(prefixes))
        for i, p in enumerate(prefixes):
            if p + "weight" not in sd:
                if p + "weight_scale" in sd:
                    raise RuntimeError(f"{p}weight_scale arrives without {p}weight")
                continue
            if parts[i] is not None or self.weight is not None:
                raise RuntimeError(f"{p}weight is loaded twice")
            w = sd[p + "weight"]
            if w.dtype != torch.float8_e4m3fn:
                raise TypeError(f"fp8 linear: {p}weight must be float8_e4m3fn, not {w.dtype}")
            if p + "weight_scale" not in sd:
                raise RuntimeError(f"{p}weight arrives without {p}weight_scale")
            scale = self._channel_scale(sd[p + "weight_scale"], w.size(0), p + "weight_scale")
            parts[i] = (self._shard(w, 0, p + "weight").to(self.device).view(torch.uint8),
                        self._shard(scale, 0, p + "weight_scale").to(self.device))
        if "weight" in self._parts and all(t is not None for t in parts):
            self._set("weight", torch.cat([w for w, _ in parts], dim=0).view(torch.float8_e4m3fn))
            self._set("weight_scale", torch.cat([s for _, s in parts], dim=0))
            del self._parts["weight"]
        if self.has_bias:
            self._load_fused(sd, prefixes, "bias")


class RowParallelFp8Linear(_Fp8LinearMixin, RowParallelLinear):
    """RowParallelLinear over an fp8 checkpoint: the weight is sharded on dim 1, the scale is whole on every rank.
    With world_size > 1 the GEMM applies the scale to this rank's partial sums, then the all-reduce, then the bias."""

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefixes=None) -> None:
        if prefixes:
            raise ValueError("row-parallel linears are never fused (parallel_linear.h:28-33)")
        self._load_one(sd, "weight", 1)
        self._load_scale(sd, self.out_features, -1)
        if self.has_bias:
            self._load_one(sd, "bias", -1)


# ---------------------------------------------------------------------------------------
# MXFP4 (e2m1 + e8m0 block scale) weight-only linear layers: W4A16 over slm_mxfp4_linear
# ---------------------------------------------------------------------------------------
class _Mxfp4LinearMixin:
    """What the two MXFP4 classes add to _LinearBase: `weight` is the checkpoint's packed tensor, uint8
    [N, K/2] (a byte's low nibble is the lower k) -- or the same bytes as [N, K/32, 16] (gpt-oss `*_blocks`) or
    torch.float4_e2m1fn_x2 -- and `weight_scale` its e8m0 bytes, uint8 or torch.float8_e8m0fnu [N, K/32]; both are
    kept as bytes and streamed as they are (kernels.mxfp4_linear).  A weight of any other dtype is an error --
    quantising is the checkpoint's job (kernels.quantize_mxfp4_weight), not a side effect of loading."""

    weight_scale: Optional[torch.Tensor] = None

    def _set(self, name: str, t: torch.Tensor) -> None:
        if name == "weight":
            t = kernels.mxfp4_bytes(t, "weight")
            if tuple(t.shape) != (self.local_out, self.local_in // 2):
                raise ValueError(f"weight size mismatch: {tuple(t.shape)} vs {(self.local_out, self.local_in // 2)}")
            self.weight = t.to(self.device).contiguous()
        elif name == "weight_scale":
            t = kernels.mxfp4_bytes(t, "weight_scale")
            if tuple(t.shape) != (self.local_out, self.local_in // 32):
                raise ValueError(f"weight_scale size mismatch: {tuple(t.shape)} vs "
                                 f"{(self.local_out, self.local_in // 32)}")
            self.weight_scale = t.to(self.device).contiguous()
        else:
            super()._set(name, t)

    def _bytes_of(self, sd: Dict[str, torch.Tensor], key: str, cols: int) -> torch.Tensor:
        """a checkpoint tensor as 2-D bytes, `cols` = its full row length"""
        t = kernels.mxfp4_bytes(sd[key], key)
        if t.dim() != 2 or t.size(1) != cols:
            raise ValueError(f"{key} size mismatch: {tuple(sd[key].shape)} for in_features {self.in_features}")
        return t

    def load_shard(self, weight: torch.Tensor, weight_scale: torch.Tensor,  # noqa: D401
                   bias: Optional[torch.Tensor] = None) -> None:
        """THIS rank's shard, already cut: packed weight [local_out, local_in / 2] and scales [local_out,
        local_in / 32]."""
        if self.weight_scale is not None:
            raise RuntimeError("weight_scale is loaded twice")
        kernels.mxfp4_bytes(weight_scale, "weight_scale")
        super().load_shard(weight, bias)
        self._set("weight_scale", weight_scale)

    def verify_loaded_weights(self, prefix: str = "") -> None:
        super().verify_loaded_weights(prefix)
        if self.weight_scale is None:
            raise RuntimeError(f"weight_scale is not loaded for {prefix}weight_scale")

    def _linear(self, x: torch.Tensor, bias: Optional[torch.Tensor], out: Optional[torch.Tensor],
                defer_splitk: bool = False) -> torch.Tensor:
        self.verify_loaded_weights()
        x2 = x.reshape(-1, x.size(-1))
        n_out = self.local_out // 2 if self.paired else self.local_out
        if out is None:
            out = torch.empty(x2.size(0), n_out, dtype=x.dtype, device=x.device)
        self.deferred = kernels.mxfp4_linear(x2, self.weight, self.weight_scale, out, bias,
                                             defer_reduce=defer_splitk and not self.paired, silu_mul=self.paired)
        self.deferred_splits = int(self.deferred)
        return out


class ColumnParallelMxfp4Linear(_Mxfp4LinearMixin, ColumnParallelLinear):
    """ColumnParallelLinear over an MXFP4 checkpoint: weight AND weight_scale are sharded on dim 0.  A fused load
    (prefixes=[...]) concatenates both tensors of the shards on dim 0 (q | k | v, gate | up)."""

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefixes=None) -> None:
        K = self.in_features
        if not prefixes:
            for name, cols in (("weight", K // 2), ("weight_scale", K // 32)):
                if name in sd:
                    if getattr(self, name) is not None:
                        raise RuntimeError(f"{name} is loaded twice")
                    self._set(name, self._shard(self._bytes_of(sd, name, cols), 0, name))
            if self.has_bias:
                self._load_one(sd, "bias", 0)
            return
        # per prefix: (weight shard, scale shard); both tensors of a prefix come together
        parts = self._parts.setdefault("weight", [None] * len(prefixes))
        for i, p in enumerate(prefixes):
            if p + "weight" not in sd:
                if p + "weight_scale" in sd:
                    raise RuntimeError(f"{p}weight_scale arrives without {p}weight")
                continue
            if parts[i] is not None or self.weight is not None:
                raise RuntimeError(f"{p}weight is loaded twice")
            w = self._bytes_of(sd, p + "weight", K // 2)
            if p + "weight_scale" not in sd:
                raise RuntimeError(f"{p}weight arrives without {p}weight_scale")
            s = self._bytes_of(sd, p + "weight_scale", K // 32)
            if s.size(0) != w.size(0):
                raise ValueError(f"{p}weight_scale has {s.size(0)} rows for {w.size(0)} weight rows")
            parts[i] = (self._shard(w, 0, p + "weight").to(self.device),
                        self._shard(s, 0, p + "weight_scale").to(self.device))
        if "weight" in self._parts and all(t is not None for t in parts):
            self._set("weight", torch.cat([w for w, _ in parts], dim=0))
            self._set("weight_scale", torch.cat([s for _, s in parts], dim=0))
            del self._parts["weight"]
        if self.has_bias:
            self._load_fused(sd, prefixes, "bias")


class RowParallelMxfp4Linear(_Mxfp4LinearMixin, RowParallelLinear):
    """RowParallelLinear over an MXFP4 checkpoint: weight and weight_scale are both sharded on dim 1 (a scale byte
    belongs to 32 k of its row), so the K shard must be a multiple of 32.  With world_size > 1: GEMM, all-reduce,
    then the bias."""

    def __init__(self, in_features, out_features, bias, input_is_parallelized, parallel_args, dtype, device):
        super().__init__(in_features, out_features, bias, input_is_parallelized, parallel_args, dtype, device)
        if self.local_in % 32:
            raise ValueError(f"mxfp4 row-parallel linear: the K shard {self.local_in} (in_features {in_features} / "
                             f"world_size {parallel_args.world_size}) must be a multiple of the MX block, 32")

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefixes=None) -> None:
        if prefixes:
            raise ValueError("row-parallel linears are never fused (parallel_linear.h:28-33)")
        K = self.in_features
        for name, cols in (("weight", K // 2), ("weight_scale", K // 32)):
            if name in sd:
                if getattr(self, name) is not None:
                    raise RuntimeError(f"{name} is loaded twice")
                self._set(name, self._shard(self._bytes_of(sd, name, cols), 1, name))
        if self.has_bias:
            self._load_one(sd, "bias", -1)


class LayerNorm:
    """llm::LayerNormImpl (normalization.h:68-110): LayerNormImpl(dim, eps, bias, options);
    forward = kernel::layer_norm on the GPU (normalization.h:86-91) -> slm_layer_norm."""

    def __init__(self, dim: int, eps: float, bias: bool, dtype: torch.dtype = torch.float16, device="cuda"):
        self.eps = float(eps)
        self.weight = torch.empty(dim, dtype=dtype, device=device)
        self.bias = torch.zeros(dim, dtype=dtype, device=device) if bias else None
        self._loaded = {"weight": False, "bias": not bias}

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor]) -> None:
        """normalization.h:98-118: copy `weight` (and `bias`) when present; shapes must match."""
        for name in ("weight", "bias"):
            t = state_dict.get(name)
            dst = getattr(self, name)
            if t is None or dst is None:
                continue
            if tuple(t.shape) != tuple(dst.shape):
                raise ValueError(f"{name} size mismatch: {tuple(t.shape)} vs {tuple(dst.shape)}")
            dst.copy_(t)
            self._loaded[name] = True

    def verify_loaded_weights(self, prefix: str = "") -> None:
        for name, ok in self._loaded.items():
            if not ok:
                raise RuntimeError(f"weight is not loaded for {prefix}{name}")

    def forward(self, input: torch.Tensor) -> torch.Tensor:  # noqa: A002 (the reference's argument name)
        out = torch.empty_like(input)
        x2 = input.view(-1, input.size(-1))
        kernels.layer_norm(out.view(-1, input.size(-1)), x2, self.weight, self.bias, self.eps)
        return out

    __call__ = forward


class GemmaRMSNorm:
    """llm::GemmaRMSNormImpl (normalization.h:142-168): GemmaRMSNormImpl(dim, eps, options); forward =
    kernel::gemma_rms_norm on the GPU -> slm_gemma_norm, form A.  `weight` is the checkpoint's (the + 1 is
    applied in the kernel, in fp32)."""

    def __init__(self, dim: int, eps: float, dtype: torch.dtype = torch.bfloat16, device="cuda"):
        self.eps = float(eps)
        self.weight = torch.empty(dim, dtype=dtype, device=device)
        self._loaded = {"weight": False}

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor]) -> None:
        t = state_dict.get("weight")
        if t is None:
            return
        if tuple(t.shape) != tuple(self.weight.shape):
            raise ValueError(f"weight size mismatch: {tuple(t.shape)} vs {tuple(self.weight.shape)}")
        self.weight.copy_(t)
        self._loaded["weight"] = True

    def verify_loaded_weights(self, prefix: str = "") -> None:
        for name, ok in self._loaded.items():
            if not ok:
                raise RuntimeError(f"weight is not loaded for {prefix}{name}")

    def forward(self, input: torch.Tensor) -> torch.Tensor:  # noqa: A002 (the reference's argument name)
        out = torch.empty_like(input)
        kernels.gemma_rms_norm(out.view(-1, input.size(-1)), input.view(-1, input.size(-1)), self.weight, self.eps)
        return out

    __call__ = forward


class Activation:
    """llm::Activation (activation.h:36-46).  The names with a custom kernel in the reference
    (gelu_new, gelu_fast, silu: activation.cpp:87-104, 117-134) run on their HIP replacements; the
    names the reference itself leaves to torch on every device (gelu, gelu_pytorch_tanh, relu) stay
    torch expressions here too -- and so does plain `silu` WITHOUT the multiply (kernel::silu,
    activation_kernels.cu:121-125), which no gated-MLP model calls: the hot path uses silu_with_mul."""

    @staticmethod
    def get_act_func(name: str):
        import torch.nn.functional as F
        n = name.lower()
        table = {"gelu_new": kernels.gelu_new, "gelu_fast": kernels.gelu_fast,
                 "gelu": F.gelu, "gelu_pytorch_tanh": lambda x: F.gelu(x, approximate="tanh"),
                 "relu": F.relu, "silu": F.silu}
        if n not in table:
            raise ValueError(f"Unsupported activation function: {name}")  # (activation.cpp:106)
        return table[n]

    @staticmethod
    def get_act_with_mul_func(name: str):
        import torch.nn.functional as F
        n = name.lower()

        def chunked(f):
            return lambda x: f(x.chunk(2, dim=-1)[0]) * x.chunk(2, dim=-1)[1]

        def silu_with_mul(x):
            out = torch.empty(x.size(0), x.size(1) // 2, dtype=x.dtype, device=x.device)
            kernels.silu_and_mul(out, x)
            return out

        table = {"gelu_new": kernels.gelu_new_with_mul, "gelu_fast": kernels.gelu_fast_with_mul,
                 "silu": silu_with_mul, "gelu": chunked(F.gelu),
                 "gelu_pytorch_tanh": chunked(lambda x: F.gelu(x, approximate="tanh")), "relu": chunked(F.relu)}
        if n not in table:
            raise ValueError(f"Unsupported activation function: {name}")
        return table[n]


# ---------------------------------------------------------------------------------------
# multi-head latent attention (DeepSeek-V2): slm_hip.h sections 18 (prologue), 10 (the two absorbed per-head
# projections as grouped GEMMs with the head as the expert) and 11 (paged attention over the latent cache)
# ---------------------------------------------------------------------------------------
class LatentKVCache:
    """The two caches of section 11 over one block pool: kv_cache [n_blocks * block_size, latent] (the normalised
    latent row, K and V at once) and k_rope_cache [n_blocks * block_size, rope] (the one rotated key per token)."""

    def __init__(self, n_blocks: int, block_size: int, latent_dim: int, rope_head_dim: int, dtype: torch.dtype,
                 device):
        self._block_size = block_size
        self.kv_cache = torch.zeros(n_blocks * block_size, latent_dim, dtype=dtype, device=device)
        self.k_rope_cache = torch.zeros(n_blocks * block_size, rope_head_dim, dtype=dtype, device=device)

    def block_size(self) -> int:
        return self._block_size

    def get_kv_cache(self) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.kv_cache, self.k_rope_cache


class MLAAttention:
    """HuggingFace DeepseekV2Attention in the ABSORBED form, on one rank:

      [q | c | k_pe] = x W^T          one column-parallel GEMM over q_proj | kv_a_proj_with_mqa, split-K deferred
                                      (with q_lora_rank: q_a_proj, q_a_layernorm, q_b_proj and kv_a_proj_with_mqa)
      prologue                        kernels.mla_rope_append: latent RMSNorm, RoPE, append into both caches
      q_lat[t, h] = q_nope[t, h] W_UK[h]          kernels.moe_grouped_gemm, the head as the expert
      out_lat = attention over the latent cache   kernels.mla_paged_kv (prefill, chunked prefill, decode)
      v[t, h] = out_lat[t, h] W_UV[h]^T           kernels.moe_grouped_gemm over kv_b_proj.weight as it is
      o = v W_o^T                                 row-parallel GEMM (split-K deferred for the caller's norm)

    kv_b_proj.weight [n_heads (nope + v), latent] is kept in T (an fp8 one is dequantised once at load): its v
    rows are used in place through a strided view, its k_nope rows transposed once into W_UK [n_heads, latent, nope].
    The grouped GEMMs need an aligned list (slm_moe_align_block of ids[t, j] = j, E = n_heads, block 32); it depends
    on the token count alone and is built once per count (prepare(T): outside a graph capture).
    quant_method "none" or "fp8" selects the classes of the other linears."""

    def __init__(self, hidden: int, n_heads: int, nope_head_dim: int, rope_head_dim: int, v_head_dim: int,
                 latent_dim: int, q_lora_rank: Optional[int], cos_sin: torch.Tensor, interleaved: bool,
                 sm_scale: float, eps: float, max_tokens: int, quant_method: str = "none",
                 parallel_args: Optional[ParallelArgs] = None, dtype: torch.dtype = torch.bfloat16, device="cuda"):
        pa = parallel_args or ParallelArgs()
        if pa.world_size > 1:
            raise ValueError("MLAAttention runs on one rank")
        if quant_method not in ("none", "fp8"):
            raise ValueError(f"quant_method must be 'none' or 'fp8', not {quant_method!r}")
        self.hidden, self.n_heads, self.nope, self.rope = hidden, n_heads, nope_head_dim, rope_head_dim
        self.v_dim, self.latent, self.q_lora_rank = v_head_dim, latent_dim, q_lora_rank
        self.cos_sin, self.interleaved, self.sm_scale, self.eps = cos_sin, interleaved, sm_scale, eps
        self.max_tokens, self.dtype, self.device, self.quant_method = max_tokens, dtype, device, quant_method
        Col, Row = (ColumnParallelFp8Linear, RowParallelFp8Linear) if quant_method == "fp8" else \
            (ColumnParallelLinear, RowParallelLinear)
        qk, H = nope_head_dim + rope_head_dim, n_heads
        self.qk = qk
        if q_lora_rank is None:
            self.qkv_a = Col(hidden, H * qk + latent_dim + rope_head_dim, False, False, pa, dtype, device)
            self.q_a = self.q_b = self.kv_a = None
        else:
            self.qkv_a = None
            self.q_a = Col(hidden, q_lora_rank, False, False, pa, dtype, device)
            self.q_b = Col(q_lora_rank, H * qk, False, False, pa, dtype, device)
            self.kv_a = Col(hidden, latent_dim + rope_head_dim, False, False, pa, dtype, device)
        self.o = Row(H * v_head_dim, hidden, False, True, pa, dtype, device)
        self.q_a_norm: Optional[torch.Tensor] = None
        self.kv_a_norm: Optional[torch.Tensor] = None
        self.kv_b: Optional[torch.Tensor] = None        # [H (nope + v), latent] T, the checkpoint tensor
        self.w_uk: Optional[torch.Tensor] = None        # [H, latent, nope] T
        self.w_uv: Optional[torch.Tensor] = None        # [H, v, latent] T: a view of kv_b
        e = lambda *s: torch.empty(*s, dtype=dtype, device=device)  # noqa: E731
        T = max_tokens
        self.buf = dict(q=e(T, H, qk), q_lat=e(T * H, latent_dim), out_lat=e(T, H, latent_dim), v=e(T * H, v_head_dim))
        if q_lora_rank is None:
            self.buf["row"] = e(T, H * qk + latent_dim + rope_head_dim)
        else:
            self.buf.update(qa=e(T, q_lora_rank), qa_n=e(T, q_lora_rank), kv_a=e(T, latent_dim + rope_head_dim))
        self._aligned: Dict[int, tuple] = {}

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """HuggingFace names relative to `self_attn.`: q_proj | q_a_proj, q_a_layernorm, q_b_proj;
        kv_a_proj_with_mqa, kv_a_layernorm, kv_b_proj, o_proj (.weight; fp8: .weight_scale beside it)."""
        sub = lambda p: {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}  # noqa: E731
        if self.qkv_a is not None:
            self.qkv_a.load_state_dict(sd, prefixes=["q_proj.", "kv_a_proj_with_mqa."])
        else:
            self.q_a.load_state_dict(sub("q_a_proj."))
            self.q_b.load_state_dict(sub("q_b_proj."))
            self.kv_a.load_state_dict(sub("kv_a_proj_with_mqa."))
            if "q_a_layernorm.weight" in sd:
                self.q_a_norm = sd["q_a_layernorm.weight"].to(self.device, self.dtype).contiguous()
        self.o.load_state_dict(sub("o_proj."))
        if "kv_a_layernorm.weight" in sd:
            self.kv_a_norm = sd["kv_a_layernorm.weight"].to(self.device, self.dtype).contiguous()
        if "kv_b_proj.weight" in sd:
            w = sd["kv_b_proj.weight"].to(self.device)
            if w.dtype == torch.float8_e4m3fn:   # dequantised once: the absorbed projections run in T
                scale = _Fp8LinearMixin._channel_scale(sd["kv_b_proj.weight_scale"], w.size(0), "kv_b weight_scale")
                w = w.float() * scale.to(self.device)[:, None]
            H, nope, v, latent = self.n_heads, self.nope, self.v_dim, self.latent
            if tuple(w.shape) != (H * (nope + v), latent):
                raise ValueError(f"kv_b_proj.weight size mismatch: {tuple(w.shape)}")
            self.kv_b = w.to(self.dtype).contiguous()
            per_head = self.kv_b.view(H, nope + v, latent)
            self.w_uk = per_head[:, :nope, :].transpose(1, 2).contiguous()
            self.w_uv = per_head[:, nope:, :]   # no copy: expert stride (nope + v) * latent, row stride latent

    def verify_loaded_weights(self) -> None:
        for lin in (self.qkv_a, self.q_a, self.q_b, self.kv_a, self.o):
            if lin is not None:
                lin.verify_loaded_weights()
        if self.kv_b is None or self.kv_a_norm is None or (self.q_a is not None and self.q_a_norm is None):
            raise RuntimeError("kv_b_proj / kv_a_layernorm / q_a_layernorm is not loaded")

    def prepare(self, n_tokens: int) -> tuple:
        """(sorted_token_idxes, expert_ids, n_padded) of the per-head grouped GEMMs for this token count: row
        t * n_heads + h belongs to expert h.  Built on first use; call it before capturing a graph."""
        if n_tokens not in self._aligned:
            H = self.n_heads
            ids = torch.arange(H, dtype=torch.int32, device=self.device).repeat(n_tokens).contiguous()
            max_padded, max_blocks = kernels.moe_align_capacity(n_tokens * H, H, kernels.MOE_GEMM_BLOCK)
            srt = torch.empty(max(max_padded, 1), dtype=torch.int32, device=self.device)
            eids = torch.empty(max(max_blocks, 1), dtype=torch.int32, device=self.device)
            n_padded = torch.zeros(1, dtype=torch.int32, device=self.device)
            kernels.moe_align_block(ids, H, kernels.MOE_GEMM_BLOCK, srt, eids, n_padded)
            self._aligned[n_tokens] = (srt, eids, n_padded)
        return self._aligned[n_tokens]

    def forward(self, x: torch.Tensor, positions: torch.Tensor, kv_cache: LatentKVCache,
                input_params: InputParameters, out: Optional[torch.Tensor] = None,
                defer_splitk: bool = False) -> torch.Tensor:
        """x [T, hidden] -> the o projection [T, hidden].  defer_splitk: the fused projection's slabs go to the
        prologue, and a split-K o projection leaves its slabs for the caller's RMSNorm (self.o.deferred is truthy
        then and the returned tensor is NOT written)."""
        T, H, b = x.size(0), self.n_heads, self.buf
        if T > self.max_tokens:
            raise kernels.SlmError(f"{T} tokens exceed max_tokens = {self.max_tokens}")
        kvc, krc = kv_cache.get_kv_cache()
        q = b["q"][:T]
        slots = input_params.new_cache_slots
        if self.qkv_a is not None:
            row = self.qkv_a.forward(x, out=b["row"][:T], defer_splitk=defer_splitk)
            part = self.qkv_a.deferred if defer_splitk else None
            if part:   # the slab form writes q whole, into the dense buffer the absorbed GEMM reads
                kernels.mla_rope_append(q, None, self.kv_a_norm, self.eps, positions, self.cos_sin, self.interleaved,
                                        slots, kvc, krc, self.nope, partials=part)
            else:      # the row was written: (t, h) rows are evenly spaced only in a dense q
                q.view(T, H * self.qk).copy_(row[:, :H * self.qk])
                kernels.mla_rope_append(q, row[:, H * self.qk:], self.kv_a_norm, self.eps, positions, self.cos_sin,
                                        self.interleaved, slots, kvc, krc, self.nope)
        else:
            qa = self.q_a.forward(x, out=b["qa"][:T])
            kernels.rms_norm(b["qa_n"][:T], qa, self.q_a_norm, self.eps)
            self.q_b.forward(b["qa_n"][:T], out=q.view(T, H * self.qk))
            kv_a = self.kv_a.forward(x, out=b["kv_a"][:T])
            kernels.mla_rope_append(q, kv_a, self.kv_a_norm, self.eps, positions, self.cos_sin, self.interleaved,
                                    slots, kvc, krc, self.nope)
        aligned = self.prepare(T)
        q_lat, out_lat, v = b["q_lat"][:T * H], b["out_lat"][:T], b["v"][:T * H]
        kernels.moe_grouped_gemm(q.view(T * H, self.qk)[:, :self.nope], self.w_uk, q_lat, *aligned, a_div=1)
        kernels.mla_paged_kv(out_lat, q_lat.view(T, H, self.latent), q[:, :, self.nope:], kvc, krc,
                             input_params.q_cu_seq_lens, input_params.kv_cu_seq_lens, input_params.block_tables,
                             input_params.cu_block_lens, kv_cache.block_size(), input_params.q_max_seq_len,
                             input_params.kv_max_seq_len, self.sm_scale)
        kernels.moe_grouped_gemm(out_lat.view(T * H, self.latent), self.w_uv, v, *aligned, a_div=1)
        return self.o.forward(v.view(T, H * self.v_dim), out=out, reduce=False, defer_splitk=defer_splitk)

    __call__ = forward
