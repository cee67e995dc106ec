"""Mixture-of-experts FFN over int4 (AWQ / GPTQ) or unquantised f16 / bf16 experts: routing, block alignment, two
grouped GEMMs and the sum over a token's experts, every step a HIP kernel of libslm_hip (include/slm_hip.h
section 10).

    FusedMoE.forward(x):  router logits (fp32, torch: [T, hidden] x [hidden, E] is tiny)
                          -> moe_topk_softmax | moe_grouped_topk_sigmoid      (weights, expert ids)
                          -> moe_align_block (32-row blocks per expert)
                          -> grouped GEMM gate_up, SiLU * mul epilogue        [T * k, intermediate]
                          -> grouped GEMM down, routing weight on the fp32 accumulator [T * k, hidden]
                          -> moe_sum                                           [T, hidden]

All buffers are sized at construction by the capacity rule (slm_moe_align_capacity) for max_tokens rows, nothing on
the path reads a device value on the host, and a smaller batch runs in views of the same buffers: forward() can be
captured in a graph and replayed for any routing.  Out of scope here: expert / tensor parallel sharding, shared
experts, 8-bit and act-order experts.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib, kernels
from .kernels import SlmError
from .layers import QuantArgs


class MoEQuantExperts:
    """The stacked packed weights of E experts: `gate_up` (w1 | w3 merged as the paired gate | up pack, K = hidden,
    N = 2 * intermediate) and `down` (w2, K = intermediate, N = hidden).  load_state_dict takes Mixtral-style names
    experts.{e}.w1|w3|w2.{qweight,qzeros,scales}; the repack is lazy, on the first forward, like the linears'."""

    def __init__(self, hidden: int, intermediate: int, n_experts: int, quant_args: QuantArgs,
                 dtype: torch.dtype, device):
        if quant_args.bits != 4:
            raise SlmError("MoE experts: 4-bit weights only (8-bit planes need the column gather)")
        if quant_args.desc_act:
            raise SlmError("MoE experts: act-order (desc_act) checkpoints are not supported")
        if quant_args.quant_method not in ("awq", "gptq"):
            raise SlmError(f"unknown quant_method {quant_args.quant_method}")
        self.hidden, self.intermediate, self.n_experts = hidden, intermediate, n_experts
        self.quant_args, self.dtype, self.device = quant_args, dtype, device
        self._ckpt: Dict[str, torch.Tensor] = {}
        self.gate_up: Optional[kernels.PackedMoeW4] = None
        self.down: Optional[kernels.PackedMoeW4] = None

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        for e in range(self.n_experts):
            for w in ("w1", "w2", "w3"):
                for name in ("qweight", "qzeros", "scales"):
                    key = f"experts.{e}.{w}.{name}"
                    if key in sd:
                        self._ckpt[key] = sd[key].to(self.device)
        self.gate_up = self.down = None

    def verify_loaded_weights(self) -> None:
        if self.gate_up is not None:
            return
        for e in range(self.n_experts):
            for w in ("w1", "w2", "w3"):
                for name in ("qweight", "qzeros", "scales"):
                    assert f"experts.{e}.{w}.{name}" in self._ckpt, f"experts.{e}.{w}.{name} is not loaded"

    def _pack_one(self, parts, paired: bool) -> kernels.PackedW4:
        # merged column-parallel weight: the checkpoint tensors concatenated along N (all three are N-minor)
        qweight = torch.cat([p["qweight"] for p in parts], dim=1).contiguous()
        qzeros = torch.cat([p["qzeros"] for p in parts], dim=1).contiguous()
        scales = torch.cat([p["scales"] for p in parts], dim=1).to(self.dtype).contiguous()
        if self.quant_args.quant_method == "awq":
            return kernels.awq_repack(qweight, qzeros, scales, self.quant_args.group_size, paired=paired)
        return kernels.gptq_repack(qweight, qzeros, scales, self.quant_args.group_size, None, paired=paired)

    def repack(self) -> None:
        self.verify_loaded_weights()
        c = self._ckpt
        get = lambda e, w: {n: c[f"experts.{e}.{w}.{n}"] for n in ("qweight", "qzeros", "scales")}  # noqa: E731
        fmt = _lib.SLM_W4_AWQ if self.quant_args.quant_method == "awq" else _lib.SLM_W4_GPTQ
        gate_up = [self._pack_one([get(e, "w1"), get(e, "w3")], True) for e in range(self.n_experts)]
        down = [self._pack_one([get(e, "w2")], False) for e in range(self.n_experts)]
        if (gate_up[0].K, gate_up[0].N) != (self.hidden, 2 * self.intermediate) or \
                (down[0].K, down[0].N) != (self.intermediate, self.hidden):
            raise SlmError("expert weights do not match hidden / intermediate")
        self.gate_up = kernels.moe_stack_experts(gate_up, fmt)
        self.down = kernels.moe_stack_experts(down, fmt)
        self._ckpt = {}

    def nbytes(self) -> int:
        return self.gate_up.nbytes() + self.down.nbytes()


class MoEDenseExperts:
    """The unquantised weights of E experts, stacked in the checkpoint's own [out, in] layout: `gate_up`
    [E, 2 * intermediate, hidden] (w1 rows, then w3 rows) and `down` [E, hidden, intermediate].  load_state_dict takes
    Mixtral-style names experts.{e}.w1|w3|w2.weight; nothing is repacked, the stacking happens on the first forward."""

    def __init__(self, hidden: int, intermediate: int, n_experts: int, dtype: torch.dtype, device):
        if dtype not in (torch.float16, torch.bfloat16):
            raise SlmError(f"MoE experts: fp16 / bf16 only, got {dtype}")
        self.hidden, self.intermediate, self.n_experts = hidden, intermediate, n_experts
        self.dtype, self.device = dtype, device
        self._ckpt: Dict[str, torch.Tensor] = {}
        self.gate_up: Optional[torch.Tensor] = None
        self.down: Optional[torch.Tensor] = None

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        for e in range(self.n_experts):
            for w in ("w1", "w2", "w3"):
                key = f"experts.{e}.{w}.weight"
                if key in sd:
                    self._ckpt[key] = sd[key].to(self.device, self.dtype)
        self.gate_up = self.down = None

    def verify_loaded_weights(self) -> None:
        if self.gate_up is not None:
            return
        for e in range(self.n_experts):
            for w in ("w1", "w2", "w3"):
                assert f"experts.{e}.{w}.weight" in self._ckpt, f"experts.{e}.{w}.weight is not loaded"

    def repack(self) -> None:
        self.verify_loaded_weights()
        c = self._ckpt
        H, I = self.hidden, self.intermediate
        for e in range(self.n_experts):
            if tuple(c[f"experts.{e}.w1.weight"].shape) != (I, H) or tuple(c[f"experts.{e}.w3.weight"].shape) != (I, H) \
                    or tuple(c[f"experts.{e}.w2.weight"].shape) != (H, I):
                raise SlmError("expert weights do not match hidden / intermediate")
        self.gate_up = torch.stack([torch.cat([c[f"experts.{e}.w1.weight"], c[f"experts.{e}.w3.weight"]], dim=0)
                                    for e in range(self.n_experts)]).contiguous()
        self.down = torch.stack([c[f"experts.{e}.w2.weight"] for e in range(self.n_experts)]).contiguous()
        self._ckpt = {}

    def nbytes(self) -> int:
        return (self.gate_up.numel() + self.down.numel()) * self.gate_up.element_size()


class FusedMoE:
    """Sparse FFN block: a router (`gate`, an unquantised [E, hidden] weight) over n_experts SwiGLU experts: int4
    (AWQ / GPTQ) with a QuantArgs, unquantised f16 / bf16 with quant_args=None.

    scoring = "softmax": top-k of the softmax (renormalize = Mixtral's rule: the k weights divided by their sum);
    scoring = "grouped_sigmoid": sigmoid scores with a correction bias, group-limited top-k (n_expert_groups,
    topk_group, scaling_factor; DeepSeek-V3 style).  max_tokens bounds the rows of one forward."""

    def __init__(self, hidden: int, intermediate: int, n_experts: int, topk: int,
                 quant_args: Optional[QuantArgs] = None,
                 scoring: str = "softmax", renormalize: bool = True, n_expert_groups: int = 1, topk_group: int = 1,
                 scaling_factor: float = 1.0, max_tokens: int = 256, dtype: torch.dtype = torch.bfloat16,
                 device="cuda"):
        if scoring not in ("softmax", "grouped_sigmoid"):
            raise SlmError(f"unknown scoring {scoring}")
        if not 1 <= topk <= n_experts:
            raise SlmError(f"topk = {topk} must be in 1 .. n_experts = {n_experts}")
        if quant_args is not None and (hidden % 128 or intermediate % 128):
            raise SlmError("hidden and intermediate must be multiples of 128 (K of the two grouped GEMMs)")
        if quant_args is None and (hidden % 32 or intermediate % 32):
            raise SlmError("hidden and intermediate must be multiples of 32 (K and N of the two grouped GEMMs)")
        self.hidden, self.intermediate, self.n_experts, self.topk = hidden, intermediate, n_experts, topk
        self.scoring, self.renormalize = scoring, renormalize
        self.n_expert_groups, self.topk_group, self.scaling_factor = n_expert_groups, topk_group, scaling_factor
        self.max_tokens, self.dtype, self.device = max_tokens, dtype, device
        self.experts = MoEDenseExperts(hidden, intermediate, n_experts, dtype, device) if quant_args is None else \
            MoEQuantExperts(hidden, intermediate, n_experts, quant_args, dtype, device)
        self._gemm = kernels.moe_grouped_gemm if quant_args is None else kernels.moe_w4_grouped_gemm
        self.gate_weight: Optional[torch.Tensor] = None       # [E, hidden]
        self.correction_bias: Optional[torch.Tensor] = None   # [E] fp32 (grouped_sigmoid)
        self._gate_f32_t: Optional[torch.Tensor] = None       # [hidden, E] fp32, built on the first forward
        self._buf = None

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        if "gate.weight" in sd:
            self.gate_weight = sd["gate.weight"].to(self.device)
            self._gate_f32_t = None
        if "gate.e_score_correction_bias" in sd:
            self.correction_bias = sd["gate.e_score_correction_bias"].to(self.device, torch.float32).contiguous()
        self.experts.load_state_dict(sd)

    def _buffers(self):
        if self._buf is None:
            n_flat = self.max_tokens * self.topk
            max_padded, max_blocks = kernels.moe_align_capacity(n_flat, self.n_experts, kernels.MOE_GEMM_BLOCK)
            dev, i32 = self.device, torch.int32
            self._buf = dict(
                weights=torch.empty(n_flat, dtype=torch.float32, device=dev),
                ids=torch.empty(n_flat, dtype=i32, device=dev),
                sorted=torch.empty(max(max_padded, 1), dtype=i32, device=dev),
                expert_ids=torch.empty(max(max_blocks, 1), dtype=i32, device=dev),
                n_padded=torch.zeros(1, dtype=i32, device=dev),
                act=torch.empty(n_flat, self.intermediate, dtype=self.dtype, device=dev),
                down=torch.empty(n_flat, self.hidden, dtype=self.dtype, device=dev),
            )
        return self._buf

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.experts.gate_up is None:
            self.experts.repack()
        if self.gate_weight is None:
            raise SlmError("gate.weight is not loaded")
        x2 = x.reshape(-1, self.hidden)
        T, k = x2.size(0), self.topk
        if T > self.max_tokens:
            raise SlmError(f"{T} tokens exceed max_tokens = {self.max_tokens} (the buffers are sized once)")
        if out is None:
            out = torch.empty(T, self.hidden, dtype=x.dtype, device=x.device)
        if T == 0:
            return out.view(x.shape)
        b = self._buffers()
        if self._gate_f32_t is None:
            self._gate_f32_t = self.gate_weight.float().t().contiguous()
        n_flat = T * k
        # the worst case for THIS batch: views of the buffers sized for max_tokens
        max_padded, max_blocks = kernels.moe_align_capacity(n_flat, self.n_experts, kernels.MOE_GEMM_BLOCK)
        weights, ids = b["weights"][:n_flat].view(T, k), b["ids"][:n_flat].view(T, k)
        srt, eids = b["sorted"][:max_padded], b["expert_ids"][:max_blocks]
        act, down = b["act"][:n_flat], b["down"][:n_flat]

        logits = x2.float() @ self._gate_f32_t
        if self.scoring == "softmax":
            kernels.moe_topk_softmax(logits, k, self.renormalize, weights, ids)
        else:
            if self.correction_bias is None:
                raise SlmError("gate.e_score_correction_bias is not loaded")
            kernels.moe_grouped_topk_sigmoid(logits, self.correction_bias, self.n_expert_groups, self.topk_group, k,
                                             self.scaling_factor, weights, ids)
        kernels.moe_align_block(ids, self.n_experts, kernels.MOE_GEMM_BLOCK, srt, eids, b["n_padded"])
        self._gemm(x2, self.experts.gate_up, act, srt, eids, b["n_padded"], a_div=k, silu_mul=True)
        self._gemm(act, self.experts.down, down, srt, eids, b["n_padded"], a_div=1, row_scale=weights.view(-1))
        kernels.moe_sum(down.view(T, k, self.hidden), out.view(T, self.hidden))
        return out.view(x.shape)

    __call__ = forward
