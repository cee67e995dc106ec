"""Mixture-of-experts FFN over int4 (AWQ / GPTQ), fp8 (e4m3, weight-only), OCP MXFP4 (weight-only) or unquantised
f16 / bf16 experts: routing, block alignment, two grouped GEMMs and the sum over a token's experts, every step a HIP
kernel of libslm_hip (include/slm_hip.h sections 10, 16 and 21).

    FusedMoE.forward(x):  router logits (fp32, torch: [T, hidden] x [hidden, E] is tiny)
                          -> moe_topk_softmax | moe_grouped_topk_sigmoid      (weights, expert ids)
                             (router="fused": both in ONE launch, kernels.moe_router, slm_hip.h section 17)
                          -> moe_align_block (32-row blocks per expert)
                          -> grouped GEMM gate_up, SiLU * mul epilogue        [T * k, intermediate]
                          -> grouped GEMM down, routing weight on the fp32 accumulator [T * k, hidden]
                          -> moe_sum                                           [T, hidden]

All buffers are sized at construction by the capacity rule (slm_moe_align_capacity) for max_tokens rows, nothing on
the path reads a device value on the host, and a smaller batch runs in views of the same buffers: forward() can be
captured in a graph and replayed for any routing.

Across GPUs the experts are sharded by expert parallelism: LocalTokenDispatcher / AlltoAllTokenDispatcher permute
tokens into expert-major rows (include/slm_hip.h section 14) and ExpertParallelMoE runs the same two grouped GEMMs
over one rank's experts between an all-to-all pair.  Out of scope here: tensor-parallel sharding of an expert,
shared experts, int8 and act-order experts, fp8 activations and block-wise fp8 scales.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import torch

from . import _lib, kernels
from .kernels import SlmError
from .layers import QuantArgs


class MoEQuantExperts:
    """The stacked packed weights of E experts: `gate_up` (w1 | w3 merged as the paired gate | up pack, K = hidden,
    N = 2 * intermediate) and `down` (w2, K = intermediate, N = hidden).  load_state_dict takes Mixtral-style names
    experts.{e}.w1|w3|w2.{qweight,qzeros,scales}; the repack is lazy, on the first forward, like the linears'."""

    def __init__(self, hidden: int, intermediate: int, n_experts: int, quant_args: QuantArgs,
                 dtype: torch.dtype, device, expert_offset: int = 0):
        if quant_args.bits != 4:
            raise SlmError("MoE experts: 4-bit weights only (8-bit planes need the column gather)")
        if quant_args.desc_act:
            raise SlmError("MoE experts: act-order (desc_act) checkpoints are not supported")
        if quant_args.quant_method not in ("awq", "gptq"):
            raise SlmError(f"unknown quant_method {quant_args.quant_method}")
        self.hidden, self.intermediate, self.n_experts = hidden, intermediate, n_experts
        self.quant_args, self.dtype, self.device = quant_args, dtype, device
        self.expert_offset = expert_offset   # expert e of this holder is experts.{expert_offset + e}.* (an EP shard)
        self._ckpt: Dict[str, torch.Tensor] = {}
        self.gate_up: Optional[kernels.PackedMoeW4] = None
        self.down: Optional[kernels.PackedMoeW4] = None

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        for e in range(self.n_experts):
            for w in ("w1", "w2", "w3"):
                for name in ("qweight", "qzeros", "scales"):
                    key = f"experts.{self.expert_offset + e}.{w}.{name}"
                    if key in sd:
                        self._ckpt[f"experts.{e}.{w}.{name}"] = sd[key].to(self.device)
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

    def gemm(self, which: str, a, c, *aligned, **epilogue) -> None:
        """the grouped GEMM over `which` = "gate_up" | "down"; the arguments after c are the kernel's"""
        kernels.moe_w4_grouped_gemm(a, getattr(self, which), c, *aligned, **epilogue)


class MoEDenseExperts:
    """The unquantised weights of E experts, stacked in the checkpoint's own [out, in] layout: `gate_up`
    [E, 2 * intermediate, hidden] (w1 rows, then w3 rows) and `down` [E, hidden, intermediate].  load_state_dict takes
    Mixtral-style names experts.{e}.w1|w3|w2.weight; nothing is repacked, the stacking happens on the first forward."""

    def __init__(self, hidden: int, intermediate: int, n_experts: int, dtype: torch.dtype, device,
                 expert_offset: int = 0):
        if dtype not in (torch.float16, torch.bfloat16):
            raise SlmError(f"MoE experts: fp16 / bf16 only, got {dtype}")
        self.hidden, self.intermediate, self.n_experts = hidden, intermediate, n_experts
        self.dtype, self.device = dtype, device
        self.expert_offset = expert_offset   # expert e of this holder is experts.{expert_offset + e}.* (an EP shard)
        self._ckpt: Dict[str, torch.Tensor] = {}
        self.gate_up: Optional[torch.Tensor] = None
        self.down: Optional[torch.Tensor] = None

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        for e in range(self.n_experts):
            for w in ("w1", "w2", "w3"):
                key = f"experts.{self.expert_offset + e}.{w}.weight"
                if key in sd:
                    self._ckpt[f"experts.{e}.{w}.weight"] = sd[key].to(self.device, self.dtype)
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

    def gemm(self, which: str, a, c, *aligned, **epilogue) -> None:
        """the grouped GEMM over `which` = "gate_up" | "down"; the arguments after c are the kernel's"""
        kernels.moe_grouped_gemm(a, getattr(self, which), c, *aligned, **epilogue)


class MoEFp8Experts:
    """The fp8 (e4m3) weights of E experts, stacked in the checkpoint's own [out, in] layout as bytes: `gate_up`
    [E, 2 * intermediate, hidden] (w1 rows, then w3 rows) and `down` [E, hidden, intermediate], with one fp32 scale
    per expert and output channel: `gate_up_scale` [E, 2 * intermediate], `down_scale` [E, hidden].  load_state_dict
    takes Mixtral-FP8 names experts.{e}.w1|w3|w2.weight (float8_e4m3fn; any other dtype is a TypeError -- nothing is
    quantised on load, as in the fp8 linears) and .weight_scale (0-d, [1], [rows] or [rows, 1], any float dtype; a
    per-tensor scale is expanded over its own rows, so w1 and w3 keep their own).  input_scale is ignored (W8A16)."""

    def __init__(self, hidden: int, intermediate: int, n_experts: int, dtype: torch.dtype, device,
                 expert_offset: int = 0):
        if dtype not in (torch.float16, torch.bfloat16):
            raise SlmError(f"MoE experts: fp16 / bf16 activations only, got {dtype}")
        self.hidden, self.intermediate, self.n_experts = hidden, intermediate, n_experts
        self.dtype, self.device = dtype, device
        self.expert_offset = expert_offset   # expert e of this holder is experts.{expert_offset + e}.* (an EP shard)
        self._ckpt: Dict[str, torch.Tensor] = {}
        self.gate_up: Optional[torch.Tensor] = None
        self.down: Optional[torch.Tensor] = None
        self.gate_up_scale: Optional[torch.Tensor] = None
        self.down_scale: Optional[torch.Tensor] = None

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        for e in range(self.n_experts):
            for w in ("w1", "w2", "w3"):
                src, dst = f"experts.{self.expert_offset + e}.{w}.", f"experts.{e}.{w}."
                if src + "weight" in sd:
                    t = sd[src + "weight"]
                    if t.dtype != torch.float8_e4m3fn:
                        raise TypeError(f"fp8 experts: {src}weight must be float8_e4m3fn, not {t.dtype} "
                                        "(quantize_fp8_weight makes one; nothing is quantised on load)")
                    self._ckpt[dst + "weight"] = t.to(self.device)
                if src + "weight_scale" in sd:
                    t = sd[src + "weight_scale"]
                    if not t.is_floating_point():
                        raise TypeError(f"{src}weight_scale must be a float tensor, not {t.dtype}")
                    self._ckpt[dst + "weight_scale"] = t.to(self.device, torch.float32)
        self.gate_up = self.down = self.gate_up_scale = self.down_scale = None

    def verify_loaded_weights(self) -> None:
        if self.gate_up is not None:
            return
        for e in range(self.n_experts):
            for w in ("w1", "w2", "w3"):
                for name in ("weight", "weight_scale"):
                    assert f"experts.{e}.{w}.{name}" in self._ckpt, f"experts.{e}.{w}.{name} is not loaded"

    @staticmethod
    def _channel_scale(t: torch.Tensor, rows: int, what: str) -> torch.Tensor:
        """0-d / [1] (per tensor) or [rows] / [rows, 1] (per channel) -> fp32 [rows]"""
        flat = t.reshape(-1)
        if flat.numel() == 1:
            return flat.expand(rows)
        if flat.numel() != rows or t.dim() > 2 or (t.dim() == 2 and t.size(1) != 1):
            raise SlmError(f"{what} size mismatch: {tuple(t.shape)} for {rows} output channels")
        return flat

    def repack(self) -> None:
        self.verify_loaded_weights()
        c = self._ckpt
        H, I = self.hidden, self.intermediate
        u8 = lambda e, w: c[f"experts.{e}.{w}.weight"].view(torch.uint8)  # noqa: E731  (cat / stack on bytes)
        sc = lambda e, w, rows: self._channel_scale(c[f"experts.{e}.{w}.weight_scale"], rows,  # noqa: E731
                                                    f"experts.{e}.{w}.weight_scale")
        for e in range(self.n_experts):
            if tuple(u8(e, "w1").shape) != (I, H) or tuple(u8(e, "w3").shape) != (I, H) or \
                    tuple(u8(e, "w2").shape) != (H, I):
                raise SlmError("expert weights do not match hidden / intermediate")
        E = range(self.n_experts)
        f8 = torch.float8_e4m3fn
        self.gate_up = torch.stack([torch.cat([u8(e, "w1"), u8(e, "w3")], dim=0) for e in E]).contiguous().view(f8)
        self.down = torch.stack([u8(e, "w2") for e in E]).contiguous().view(f8)
        self.gate_up_scale = torch.stack([torch.cat([sc(e, "w1", I), sc(e, "w3", I)]) for e in E]).contiguous()
        self.down_scale = torch.stack([sc(e, "w2", H) for e in E]).contiguous()
        self._ckpt = {}

    def nbytes(self) -> int:
        return self.gate_up.numel() + self.down.numel() + 4 * (self.gate_up_scale.numel() + self.down_scale.numel())

    def gemm(self, which: str, a, c, *aligned, **epilogue) -> None:
        """the grouped GEMM over `which` = "gate_up" | "down"; the arguments after c are the kernel's"""
        kernels.moe_fp8_grouped_gemm(a, getattr(self, which), getattr(self, which + "_scale"), c, *aligned,
                                     **epilogue)


class MoEMxfp4Experts:
    """The OCP MXFP4 weights of E experts, stacked in the checkpoint's own [out, in] layout as bytes of two e2m1 codes
    (low nibble = lower k) with one e8m0 scale byte per 32 k: `gate_up` uint8 [E, 2 * intermediate, hidden / 2] (w1
    rows, then w3 rows) + `gate_up_scale` uint8 [E, 2 * intermediate, hidden / 32]; `down` [E, hidden,
    intermediate / 2] + `down_scale` [E, hidden, intermediate / 32].  load_state_dict takes the Quark names
    experts.{e}.w1|w3|w2.weight (uint8, or float4_e2m1fn_x2 / the [rows, K/32, 16] blocks form) and .weight_scale
    (uint8 or float8_e8m0fnu), both through kernels.mxfp4_bytes: any other dtype is a TypeError -- nothing is quantised
    on load, as in the MXFP4 linears."""

    def __init__(self, hidden: int, intermediate: int, n_experts: int, dtype: torch.dtype, device,
                 expert_offset: int = 0):
        if dtype not in (torch.float16, torch.bfloat16):
            raise SlmError(f"MoE experts: fp16 / bf16 activations only, got {dtype}")
        self.hidden, self.intermediate, self.n_experts = hidden, intermediate, n_experts
        self.dtype, self.device = dtype, device
        self.expert_offset = expert_offset   # expert e of this holder is experts.{expert_offset + e}.* (an EP shard)
        self._ckpt: Dict[str, torch.Tensor] = {}
        self.gate_up: Optional[torch.Tensor] = None
        self.down: Optional[torch.Tensor] = None
        self.gate_up_scale: Optional[torch.Tensor] = None
        self.down_scale: Optional[torch.Tensor] = None

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        for e in range(self.n_experts):
            for w in ("w1", "w2", "w3"):
                src, dst = f"experts.{self.expert_offset + e}.{w}.", f"experts.{e}.{w}."
                for name in ("weight", "weight_scale"):
                    if src + name in sd:
                        self._ckpt[dst + name] = kernels.mxfp4_bytes(sd[src + name], src + name).to(self.device)
        self.gate_up = self.down = self.gate_up_scale = self.down_scale = None

    def verify_loaded_weights(self) -> None:
        if self.gate_up is not None:
            return
        for e in range(self.n_experts):
            for w in ("w1", "w2", "w3"):
                for name in ("weight", "weight_scale"):
                    assert f"experts.{e}.{w}.{name}" in self._ckpt, f"experts.{e}.{w}.{name} is not loaded"

    def repack(self) -> None:
        self.verify_loaded_weights()
        c = self._ckpt
        H, I, B = self.hidden, self.intermediate, kernels.MXFP4_BLOCK
        for e in range(self.n_experts):
            for w, rows, k in (("w1", I, H), ("w3", I, H), ("w2", H, I)):
                if tuple(c[f"experts.{e}.{w}.weight"].shape) != (rows, k // 2) or \
                        tuple(c[f"experts.{e}.{w}.weight_scale"].shape) != (rows, k // B):
                    raise SlmError(f"experts.{e}.{w}: weight must be [{rows}, {k // 2}] bytes and weight_scale "
                                   f"[{rows}, {k // B}] (hidden = {H}, intermediate = {I})")
        E = range(self.n_experts)
        cat = lambda e, name: torch.cat([c[f"experts.{e}.w1.{name}"], c[f"experts.{e}.w3.{name}"]], dim=0)  # noqa: E731
        self.gate_up = torch.stack([cat(e, "weight") for e in E]).contiguous()
        self.gate_up_scale = torch.stack([cat(e, "weight_scale") for e in E]).contiguous()
        self.down = torch.stack([c[f"experts.{e}.w2.weight"] for e in E]).contiguous()
        self.down_scale = torch.stack([c[f"experts.{e}.w2.weight_scale"] for e in E]).contiguous()
        self._ckpt = {}

    def nbytes(self) -> int:
        return self.gate_up.numel() + self.down.numel() + self.gate_up_scale.numel() + self.down_scale.numel()

    def gemm(self, which: str, a, c, *aligned, **epilogue) -> None:
        """the grouped GEMM over `which` = "gate_up" | "down"; the arguments after c are the kernel's"""
        kernels.moe_mxfp4_grouped_gemm(a, getattr(self, which), getattr(self, which + "_scale"), c, *aligned,
                                       **epilogue)


def _make_experts(hidden: int, intermediate: int, n_experts: int, quant_args: Optional[QuantArgs], dtype, device,
                  expert_offset: int = 0):
    """The experts holder a QuantArgs selects: None -> unquantised, "fp8" -> MoEFp8Experts, "mxfp4" ->
    MoEMxfp4Experts, else int4."""
    if quant_args is None or quant_args.quant_method in ("fp8", "mxfp4"):
        if quant_args is not None and quant_args.quant_method == "fp8" and quant_args.bits != 8:
            raise SlmError(f"quant_method 'fp8' means 8-bit weights, got bits = {quant_args.bits}")
        if quant_args is not None and quant_args.quant_method == "mxfp4" and quant_args.bits != 4:
            raise SlmError(f"quant_method 'mxfp4' means 4-bit weights, got bits = {quant_args.bits}")
        if hidden % 32 or intermediate % 32:
            raise SlmError("hidden and intermediate must be multiples of 32 (K and N of the two grouped GEMMs)")
        cls = MoEDenseExperts if quant_args is None else \
            MoEFp8Experts if quant_args.quant_method == "fp8" else MoEMxfp4Experts
        return cls(hidden, intermediate, n_experts, dtype, device, expert_offset)
    if hidden % 128 or intermediate % 128:
        raise SlmError("hidden and intermediate must be multiples of 128 (K of the two grouped GEMMs)")
    return MoEQuantExperts(hidden, intermediate, n_experts, quant_args, dtype, device, expert_offset)


class FusedMoE:
    """Sparse FFN block: a router (`gate`, an unquantised [E, hidden] weight) over n_experts SwiGLU experts: int4
    (AWQ / GPTQ) with a QuantArgs, fp8 (e4m3 weights, f16 / bf16 activations) with QuantArgs("fp8", 8), OCP MXFP4
    (e2m1 nibbles + e8m0 block scales, f16 / bf16 activations) with QuantArgs("mxfp4", 4) -- the other fields of
    these two are ignored --, unquantised f16 / bf16 with quant_args=None.  Each experts class runs its own grouped
    GEMM (experts.gemm); the forward pass is the same six launches for all four.

    scoring = "softmax": top-k of the softmax (renormalize = Mixtral's rule: the k weights divided by their sum);
    scoring = "grouped_sigmoid": sigmoid scores with a correction bias, group-limited top-k (n_expert_groups,
    topk_group, scaling_factor; DeepSeek-V3 style).  max_tokens bounds the rows of one forward."""

    def __init__(self, hidden: int, intermediate: int, n_experts: int, topk: int,
                 quant_args: Optional[QuantArgs] = None,
                 scoring: str = "softmax", renormalize: bool = True, n_expert_groups: int = 1, topk_group: int = 1,
                 scaling_factor: float = 1.0, max_tokens: int = 256, dtype: torch.dtype = torch.bfloat16,
                 device="cuda", router: str = "torch"):
        if scoring not in ("softmax", "grouped_sigmoid"):
            raise SlmError(f"unknown scoring {scoring}")
        if router not in ("torch", "fused"):
            raise SlmError(f"unknown router {router}: 'torch' or 'fused'")
        self.router = router
        if not 1 <= topk <= n_experts:
            raise SlmError(f"topk = {topk} must be in 1 .. n_experts = {n_experts}")
        self.hidden, self.intermediate, self.n_experts, self.topk = hidden, intermediate, n_experts, topk
        self.scoring, self.renormalize = scoring, renormalize
        self.n_expert_groups, self.topk_group, self.scaling_factor = n_expert_groups, topk_group, scaling_factor
        self.max_tokens, self.dtype, self.device = max_tokens, dtype, device
        self.experts = _make_experts(hidden, intermediate, n_experts, quant_args, dtype, device)
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

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None,
                router_logits_out: Optional[torch.Tensor] = None,
                shared_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """router_logits_out (router="fused" only): contiguous fp32 [T, n_experts] that receives the router logits.
        shared_out: contiguous [T, hidden], the output of the always-on shared experts (DeepSeek) for the same rows;
        it is added to the routed sum in the final launch (kernels.moe_sum_add: fp32, after the k routed rows, one
        rounding) instead of in a launch of its own.  It may be `out`."""
        if router_logits_out is not None and self.router != "fused":
            raise SlmError("router_logits_out needs router='fused'")
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
        if shared_out is not None and (shared_out.numel() != T * self.hidden or shared_out.dtype != x.dtype or
                                       not shared_out.is_contiguous()):
            raise SlmError("shared_out must be a contiguous [T, hidden] tensor of the activations' dtype")
        if T == 0:
            return out.view(x.shape)
        b = self._buffers()
        n_flat = T * k
        # the worst case for THIS batch: views of the buffers sized for max_tokens
        max_padded, max_blocks = kernels.moe_align_capacity(n_flat, self.n_experts, kernels.MOE_GEMM_BLOCK)
        weights, ids = b["weights"][:n_flat].view(T, k), b["ids"][:n_flat].view(T, k)
        srt, eids = b["sorted"][:max_padded], b["expert_ids"][:max_blocks]
        act, down = b["act"][:n_flat], b["down"][:n_flat]

        if self.scoring != "softmax" and self.correction_bias is None:
            raise SlmError("gate.e_score_correction_bias is not loaded")
        if self.router == "fused":   # gate GEMM + routing: one launch, no fp32 copy of the gate
            kernels.moe_router(x2, self.gate_weight, k, scoring=self.scoring, renormalize=self.renormalize,
                               correction_bias=self.correction_bias if self.scoring != "softmax" else None,
                               n_expert_groups=self.n_expert_groups, topk_group=self.topk_group,
                               scaling_factor=self.scaling_factor, weights=weights, indices=ids,
                               logits_out=router_logits_out)
        else:
            if self._gate_f32_t is None:
                self._gate_f32_t = self.gate_weight.float().t().contiguous()
            logits = x2.float() @ self._gate_f32_t
            if self.scoring == "softmax":
                kernels.moe_topk_softmax(logits, k, self.renormalize, weights, ids)
            else:
                kernels.moe_grouped_topk_sigmoid(logits, self.correction_bias, self.n_expert_groups, self.topk_group,
                                                 k, self.scaling_factor, weights, ids)
        kernels.moe_align_block(ids, self.n_experts, kernels.MOE_GEMM_BLOCK, srt, eids, b["n_padded"])
        self.experts.gemm("gate_up", x2, act, srt, eids, b["n_padded"], a_div=k, silu_mul=True)
        self.experts.gemm("down", act, down, srt, eids, b["n_padded"], a_div=1, row_scale=weights.view(-1))
        if shared_out is None:
            kernels.moe_sum(down.view(T, k, self.hidden), out.view(T, self.hidden))
        else:
            kernels.moe_sum_add(down.view(T, k, self.hidden), shared_out.view(T, self.hidden),
                                out.view(T, self.hidden))
        return out.view(x.shape)

    __call__ = forward


# ---------------------------------------------------------------------------------------------------------------
# Token dispatchers (reference src/layers/moe/): tokens -> expert-major rows -> (experts) -> tokens, on one GPU
# (LocalTokenDispatcher) or across an expert-parallel group (AlltoAllTokenDispatcher).  Both keep the row_id_map
# and the probabilities between dispatch and combine; the probability multiply is part of the un-permute kernel.
#   dispatch(tokens, probs [T, E], routing_map [T, E] bool)      the reference's entry (mask-map kernels)
#   dispatch_topk(tokens, topk_weights [T, k], topk_ids [T, k])  what moe_topk_softmax produces (index-map kernels)
# ---------------------------------------------------------------------------------------------------------------
class AlltoAllPlan(NamedTuple):
    input_split_sizes: List[int]             # rows this rank sends to each rank
    output_split_sizes: List[int]            # rows it receives from each rank
    tokens_per_local_expert: torch.Tensor    # [n_local_experts] int64 (CPU): rows per expert of this rank
    reorder: Optional[torch.Tensor]          # [rows received] int32 (CPU): received row (rank, expert)-major ->
    #                                          its row in (expert, rank) order; None when that is the identity


def alltoall_plan(counts, rank: int) -> AlltoAllPlan:
    """The bookkeeping of alltoall_token_dispatcher.cpp:148-189 as a pure function of the gathered counts
    [ep, n_experts] (row r = rank r's tokens per expert) and this rank.  Ranks own contiguous expert ranges."""
    counts = torch.as_tensor(counts, dtype=torch.int64, device="cpu")
    ep, E = counts.shape
    if E % ep:
        raise SlmError("n_experts must be divisible by the expert-parallel size")
    L = E // ep
    local = counts[:, rank * L:(rank + 1) * L]                        # [ep, L]: what each rank sends here
    plan = AlltoAllPlan(counts[rank].view(ep, L).sum(1).tolist(), local.sum(1).tolist(), local.sum(0), None)
    if ep == 1 or L == 1:
        return plan
    src = local.reshape(-1)                                           # chunk sizes as received: (rank, expert)
    src_off = src.cumsum(0) - src
    dst = local.t().reshape(-1)                                       # ... as the grouped GEMM wants: (expert, rank)
    dst_off = (dst.cumsum(0) - dst).view(L, ep).t().reshape(-1)       # indexed like src
    chunk = torch.repeat_interleave(torch.arange(ep * L), src)
    reorder = (dst_off - src_off)[chunk] + torch.arange(chunk.numel())
    return plan._replace(reorder=reorder.to(torch.int32))


class _TokenDispatcher:
    """State shared by both dispatchers: the map, the probabilities and the shape to restore."""

    def __init__(self, topk: int, n_experts: Optional[int] = None):
        self.topk, self.n_experts = topk, n_experts
        self._map = self._probs = self._shape = None

    @staticmethod
    def _check_tokens(tokens: torch.Tensor) -> None:
        if tokens.dim() != 2 or not tokens.is_contiguous():
            raise SlmError("tokens must be a contiguous [n_tokens, dim] tensor")

    def _map_mask(self, tokens, probs, routing_map):
        self._check_tokens(tokens)
        if tuple(probs.shape) != tuple(routing_map.shape) or routing_map.size(0) != tokens.size(0):
            raise SlmError("probs and routing_map must be [n_tokens, n_experts]")
        if self.n_experts is not None and routing_map.size(1) != self.n_experts:
            raise SlmError(f"routing_map has {routing_map.size(1)} experts, the dispatcher {self.n_experts}")
        self._map, counts = kernels.permute_mask_map(routing_map, count=True)
        self._probs, self._shape = probs.contiguous(), tokens.shape
        return counts

    def _map_index(self, tokens, topk_weights, topk_ids):
        self._check_tokens(tokens)
        if self.n_experts is None:
            raise SlmError("dispatch_topk needs the dispatcher built with n_experts")
        if tuple(topk_ids.shape) != (tokens.size(0), self.topk) or tuple(topk_weights.shape) != tuple(topk_ids.shape):
            raise SlmError("topk_weights and topk_ids must be [n_tokens, topk]")
        self._map, counts = kernels.permute_index_map(topk_ids, self.n_experts, count=True)
        self._probs, self._shape = topk_weights.contiguous(), tokens.shape
        return counts

    def _permute(self, tokens: torch.Tensor) -> torch.Tensor:
        out = torch.empty(tokens.size(0) * self.topk, tokens.size(1), dtype=tokens.dtype, device=tokens.device)
        return kernels.permute_rows(tokens, self._map, out)

    def _unpermute(self, permuted: torch.Tensor) -> torch.Tensor:
        if self._map is None:
            raise SlmError("combine() without a dispatch before it")
        return kernels.unpermute_rows(permuted, self._map, self._probs, self._shape[0]).view(self._shape)


class LocalTokenDispatcher(_TokenDispatcher):
    """llm::LocalTokenDispatcher: every expert lives on this GPU.  dispatch returns (permuted_tokens [T * topk, dim]
    sorted by expert, tokens_per_expert [E] int32 from the map kernel); combine(permuted) returns the tokens'
    weighted sums in their first order (bias is accepted and unused, as in the reference).  T * topk is known on
    the host, so nothing is read back and dispatch -> experts -> combine can be captured in a graph.  Rows past the
    mapped count (a routing_map row with fewer than topk experts, an id outside [0, n_experts)) are not written."""

    def dispatch(self, tokens, probs, routing_map):
        counts = self._map_mask(tokens, probs, routing_map)
        return self._permute(tokens), counts

    def dispatch_topk(self, tokens, topk_weights, topk_ids):
        counts = self._map_index(tokens, topk_weights, topk_ids)
        return self._permute(tokens), counts

    def combine(self, permuted_tokens, bias=None):
        return self._unpermute(permuted_tokens)


class AlltoAllTokenDispatcher(_TokenDispatcher):
    """llm::AlltoAllTokenDispatcher (alltoall_token_dispatcher.cpp:126-253): rank r of the expert-parallel group owns
    experts [r * L, (r + 1) * L), L = n_experts / ep.  dispatch: per-expert counts from the map kernel -> all-gather
    -> split sizes -> permute -> all-to-all -> (rank, expert) to (expert, rank) chunk reorder when L > 1; returns
    (the rows of this rank's experts sorted by expert, tokens_per_local_expert [L] int32).  combine is the inverse,
    ending in the probability-weighted un-permute.

    The gathered counts are copied to the host once per dispatch (the split sizes of the all-to-all are host
    integers; the reference does the same), so this class canNOT be captured in a graph.  That copy is its only
    device-to-host transfer.  With ep == 1 nothing is gathered or copied."""

    def __init__(self, n_experts: int, topk: int, process_group):
        super().__init__(topk, n_experts)
        self.pg = process_group
        self.ep_size, self.ep_rank = process_group.world_size, process_group.rank
        if n_experts % self.ep_size:
            raise SlmError("n_experts must be divisible by the expert-parallel size")
        self.n_local_experts = n_experts // self.ep_size
        self._plan: Optional[AlltoAllPlan] = None
        self._reorder = None

    def _gather_plan(self, counts: torch.Tensor) -> AlltoAllPlan:
        """all-gather this rank's per-expert counts and plan the exchange from every rank's"""
        gathered = torch.empty(self.ep_size * self.n_experts, dtype=torch.int32, device=counts.device)
        self.pg.allgather_into(counts, gathered)
        return alltoall_plan(gathered.cpu().view(self.ep_size, -1), self.ep_rank)   # THE device-to-host copy

    def _exchange(self, tokens: torch.Tensor, counts: torch.Tensor):
        permuted = self._permute(tokens)
        if self.ep_size == 1:
            return permuted, counts
        plan = self._plan = self._gather_plan(counts)
        n_send, n_recv = sum(plan.input_split_sizes), sum(plan.output_split_sizes)
        recv = torch.empty(n_recv, tokens.size(1), dtype=tokens.dtype, device=tokens.device)
        self.pg.alltoall(permuted[:n_send], recv, plan.input_split_sizes, plan.output_split_sizes)
        self._reorder = None
        if plan.reorder is not None and n_recv:
            self._reorder = plan.reorder.to(tokens.device)
            recv = kernels.permute_rows(recv, self._reorder, torch.empty_like(recv))
        return recv, plan.tokens_per_local_expert.to(device=tokens.device, dtype=torch.int32)

    def dispatch(self, tokens, probs, routing_map):
        return self._exchange(tokens, self._map_mask(tokens, probs, routing_map))

    def dispatch_topk(self, tokens, topk_weights, topk_ids):
        return self._exchange(tokens, self._map_index(tokens, topk_weights, topk_ids))

    def combine(self, permuted_tokens, bias=None):
        if self.ep_size == 1:
            return self._unpermute(permuted_tokens)
        plan = self._plan
        if plan is None:
            raise SlmError("combine() without a dispatch before it")
        if self._reorder is not None:   # back to (rank, expert) order: row i comes from row reorder[i]
            permuted_tokens = kernels.unpermute_rows(permuted_tokens, self._reorder, None, permuted_tokens.size(0))
        back = torch.empty(sum(plan.input_split_sizes), permuted_tokens.size(1), dtype=permuted_tokens.dtype,
                           device=permuted_tokens.device)
        self.pg.alltoall(permuted_tokens, back, plan.output_split_sizes, plan.input_split_sizes)
        return self._unpermute(back)


class ExpertParallelMoE:
    """FusedMoE's block with the experts sharded over an expert-parallel group: every rank routes its own tokens
    (the router weight is replicated), AlltoAllTokenDispatcher.dispatch_topk sends each (token, expert) row to the
    expert's rank, the two grouped GEMMs run over this rank's experts [rank * L, (rank + 1) * L) (any of FusedMoE's
    expert sides: quant_args as there, QuantArgs("mxfp4", 4) included), and combine
    brings the rows home and takes the weighted sum.  Rounding points: after SiLU * mul, after the down GEMM (the
    rows travel in T), after the weighted sum (fp32, one rounding) -- the weights are applied at the source rank,
    not on the down GEMM's accumulator as in FusedMoE.  Not capturable (the dispatcher's copy of the counts)."""

    def __init__(self, hidden: int, intermediate: int, n_experts: int, topk: int, process_group,
                 quant_args: Optional[QuantArgs] = None, scoring: str = "softmax", renormalize: bool = True,
                 n_expert_groups: int = 1, topk_group: int = 1, scaling_factor: float = 1.0,
                 dtype: torch.dtype = torch.bfloat16, device="cuda", router: str = "torch"):
        if scoring not in ("softmax", "grouped_sigmoid"):
            raise SlmError(f"unknown scoring {scoring}")
        if router not in ("torch", "fused"):
            raise SlmError(f"unknown router {router}: 'torch' or 'fused'")
        self.router = router
        if not 1 <= topk <= n_experts:
            raise SlmError(f"topk = {topk} must be in 1 .. n_experts = {n_experts}")
        self.dispatcher = AlltoAllTokenDispatcher(n_experts, topk, process_group)
        L = self.n_local_experts = self.dispatcher.n_local_experts
        self.hidden, self.intermediate, self.n_experts, self.topk = hidden, intermediate, n_experts, topk
        self.scoring, self.renormalize = scoring, renormalize
        self.n_expert_groups, self.topk_group, self.scaling_factor = n_expert_groups, topk_group, scaling_factor
        self.dtype, self.device = dtype, device
        offset = process_group.rank * L
        self.experts = _make_experts(hidden, intermediate, L, quant_args, dtype, device, expert_offset=offset)
        self.gate_weight: Optional[torch.Tensor] = None
        self.correction_bias: Optional[torch.Tensor] = None
        self._gate_f32_t: Optional[torch.Tensor] = None

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        if "gate.weight" in sd:
            self.gate_weight = sd["gate.weight"].to(self.device)
            self._gate_f32_t = None
        if "gate.e_score_correction_bias" in sd:
            self.correction_bias = sd["gate.e_score_correction_bias"].to(self.device, torch.float32).contiguous()
        self.experts.load_state_dict(sd)

    def _experts_forward(self, rows: torch.Tensor, tokens_per_local_expert: torch.Tensor) -> torch.Tensor:
        n, L, dev, i32 = rows.size(0), self.n_local_experts, rows.device, torch.int32
        down = torch.empty(n, self.hidden, dtype=rows.dtype, device=dev)
        if n == 0:
            return down
        # the expert of every row (the rows are sorted by expert), aligned to the GEMM's blocks as topk = 1 ids
        row_expert = torch.repeat_interleave(torch.arange(L, dtype=i32, device=dev), tokens_per_local_expert,
                                             output_size=n).to(i32).view(n, 1).contiguous()
        max_padded, max_blocks = kernels.moe_align_capacity(n, L, kernels.MOE_GEMM_BLOCK)
        srt = torch.empty(max_padded, dtype=i32, device=dev)
        eids = torch.empty(max_blocks, dtype=i32, device=dev)
        n_padded = torch.zeros(1, dtype=i32, device=dev)
        kernels.moe_align_block(row_expert, L, kernels.MOE_GEMM_BLOCK, srt, eids, n_padded)
        act = torch.empty(n, self.intermediate, dtype=rows.dtype, device=dev)
        self.experts.gemm("gate_up", rows, act, srt, eids, n_padded, a_div=1, silu_mul=True)
        self.experts.gemm("down", act, down, srt, eids, n_padded, a_div=1)
        return down

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.experts.gate_up is None:
            self.experts.repack()
        if self.gate_weight is None:
            raise SlmError("gate.weight is not loaded")
        x2 = x.reshape(-1, self.hidden).contiguous()
        if self.scoring != "softmax" and self.correction_bias is None:
            raise SlmError("gate.e_score_correction_bias is not loaded")
        if self.router == "fused":
            weights, ids = kernels.moe_router(
                x2, self.gate_weight, self.topk, scoring=self.scoring, renormalize=self.renormalize,
                correction_bias=self.correction_bias if self.scoring != "softmax" else None,
                n_expert_groups=self.n_expert_groups, topk_group=self.topk_group, scaling_factor=self.scaling_factor)
        else:
            if self._gate_f32_t is None:
                self._gate_f32_t = self.gate_weight.float().t().contiguous()
            logits = x2.float() @ self._gate_f32_t
            if self.scoring == "softmax":
                weights, ids = kernels.moe_topk_softmax(logits, self.topk, self.renormalize)
            else:
                weights, ids = kernels.moe_grouped_topk_sigmoid(logits, self.correction_bias, self.n_expert_groups,
                                                                self.topk_group, self.topk, self.scaling_factor)
        rows, tokens_per_local_expert = self.dispatcher.dispatch_topk(x2, weights, ids)
        return self.dispatcher.combine(self._experts_forward(rows, tokens_per_local_expert)).view(x.shape)

    __call__ = forward
