"""A DeepSeek-V2-shaped decode step on the fused path, beside mixtral.MixtralDecodeStep and on its contract: seeded
synthetic checkpoint (keep_checkpoint: HuggingFace names), record_routing, static buffers, forward(tokens, positions,
params, return_logits, sampling), capturable with torch.cuda.graph on one stream, one lane, one rank.  Per layer
(HuggingFace DeepseekV2DecoderLayer):

  input norm (fused into the previous layer's residual add)                    kernels.rms_norm(residual=)
  multi-head latent attention, absorbed form                                   layers.MLAAttention:
    [q | c | k_pe] GEMM (split-K slabs deferred) -> latent norm + RoPE + append in ONE launch (slm_mla_rope_append)
    -> q W_UK per head (grouped GEMM) -> paged attention over the latent cache -> W_UV per head (grouped GEMM)
    -> o GEMM (deferred) -> residual + post-attention norm                     kernels.rms_norm(residual=, partials=)
  layers below first_k_dense_replace: dense SwiGLU MLP, SiLU * mul in the gate_up GEMM's epilogue
  the others: the shared experts as ONE dense MLP of width n_shared * moe_intermediate, then the routed experts
    (moe.FusedMoE, router="fused": softmax, top-k; norm_topk_prob -> renormalize), whose final sum takes the
    shared output as one more row (slm_moe_sum_add): no separate add                     FusedMoE(shared_out=)
  residual + the next layer's input norm (or the final norm)
  untied lm_head -> argmax, or the fused sampling kernel

RoPE pairs (2i, 2i + 1) as HuggingFace's DeepSeek-V2 does.  rope_type "default", or "yarn" as a host-built table:
inv_freq and the attention factor as transformers' yarn init computes them (rope_cos_sin_table; the factor is folded
into cos | sin), and mscale_all_dim folded into sm_scale (attention_sm_scale).

quant_method "none" (f16 / bf16) or "fp8" (e4m3 weights with channel scales, W8A16) for every linear and the
experts; kv_b_proj is dequantised once at load and runs in T, gate.weight stays in T.

Routing is topk_method "greedy".  "group_limited_greedy" scores a group by its MAXIMUM, which the routing kernels
(slm_hip.h section 10: sum of the two largest) do not offer: refused.  routed_scaling_factor multiplies the routing
weights; folding it into a weight tensor would round those weights a second time, so a factor other than 1 is
refused as well.

Out of scope: tensor / expert parallelism (world_size > 1 is refused), int4 weights, a C++ host step, DeepSeek-V3
(sigmoid routing exists in the kernels but is not wired here), an fp8 latent cache.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import kernels
from .layers import (ColumnParallelFp8Linear, ColumnParallelLinear, HipAttnHandler, InputParameters, LatentKVCache,
                     MLAAttention, QuantArgs, RowParallelFp8Linear, RowParallelLinear)
from .model_parallel import ParallelArgs
from .moe import FusedMoE


@dataclass
class DeepseekV2Shape:
    hidden: int = 2048
    n_heads: int = 16
    nope_head_dim: int = 128
    rope_head_dim: int = 64
    v_head_dim: int = 128
    kv_lora_rank: int = 512
    q_lora_rank: Optional[int] = None
    intermediate: int = 10944
    moe_intermediate: int = 1408
    n_routed_experts: int = 64
    n_shared_experts: int = 2
    topk: int = 6
    first_k_dense_replace: int = 1
    n_layers: int = 27
    vocab: int = 102400
    rms_eps: float = 1e-6
    rope_theta: float = 10000.0
    max_position: int = 4096
    norm_topk_prob: bool = False
    routed_scaling_factor: float = 1.0
    topk_method: str = "greedy"
    rope_type: str = "default"           # or "yarn"
    rope_factor: float = 1.0             # yarn: the context extension factor
    original_max_position: int = 4096    # yarn
    beta_fast: float = 32.0
    beta_slow: float = 1.0
    mscale: float = 1.0
    mscale_all_dim: float = 0.0

    @staticmethod
    def tiny() -> "DeepseekV2Shape":
        """every size is accepted by the dense / fp8 grouped GEMMs (% 32) and by section 11 (latent 128, rope 64)"""
        return DeepseekV2Shape(hidden=256, n_heads=4, nope_head_dim=32, rope_head_dim=64, v_head_dim=32,
                               kv_lora_rank=128, q_lora_rank=None, intermediate=512, moe_intermediate=128,
                               n_routed_experts=8, n_shared_experts=2, topk=3, first_k_dense_replace=1, n_layers=3,
                               vocab=1024, max_position=512)

    @staticmethod
    def tiny_qlora() -> "DeepseekV2Shape":
        s = DeepseekV2Shape.tiny()
        s.q_lora_rank = 64
        return s

    @staticmethod
    def v2_lite() -> "DeepseekV2Shape":
        """UNVERIFIED: written from memory of the public deepseek-ai/DeepSeek-V2-Lite config.json, which was not at
        hand to check against; compare with the checkpoint's own config before relying on it"""
        return DeepseekV2Shape(max_position=163840, rope_type="yarn", rope_factor=40.0, original_max_position=4096,
                               beta_fast=32.0, beta_slow=1.0, mscale=0.707, mscale_all_dim=0.707)


def _yarn_mscale(scale: float, mscale: float = 1.0) -> float:
    return 1.0 if scale <= 1 else 0.1 * mscale * math.log(scale) + 1.0


def yarn_inv_freq(shape: DeepseekV2Shape, device=None):
    """(inv_freq [rope / 2] fp32, attention factor): transformers' _compute_yarn_parameters restated for the rope
    columns of DeepSeek-V2 (dim = rope_head_dim, truncated correction range)"""
    dim, base, factor = shape.rope_head_dim, shape.rope_theta, shape.rope_factor
    if shape.mscale and shape.mscale_all_dim:
        attention_factor = float(_yarn_mscale(factor, shape.mscale) / _yarn_mscale(factor, shape.mscale_all_dim))
    else:
        attention_factor = _yarn_mscale(factor)

    def correction_dim(n_rot):
        return (dim * math.log(shape.original_max_position / (n_rot * 2 * math.pi))) / (2 * math.log(base))

    low, high = max(math.floor(correction_dim(shape.beta_fast)), 0), min(math.ceil(correction_dim(shape.beta_slow)),
                                                                         dim - 1)
    if low == high:
        high += 0.001
    pos_freqs = base ** (torch.arange(0, dim, 2, device=device, dtype=torch.float32) / dim)
    extrapolation, interpolation = 1.0 / pos_freqs, 1.0 / (factor * pos_freqs)
    ramp = torch.clamp((torch.arange(dim // 2, dtype=torch.float32, device=device) - low) / (high - low), 0, 1)
    keep = 1 - ramp
    return interpolation * (1 - keep) + extrapolation * keep, attention_factor


def rope_cos_sin_table(shape: DeepseekV2Shape, device=None) -> torch.Tensor:
    """[max_position, rope] = cos | sin in fp32 (section 5's row layout).  yarn: the blended frequencies, and the
    attention factor multiplied into both halves, as DeepseekV2RotaryEmbedding scales its freqs_cis."""
    if shape.rope_type == "default":
        dim = shape.rope_head_dim
        inv = 1.0 / (shape.rope_theta ** (torch.arange(0, dim, 2, dtype=torch.float32, device=device) / dim))
        return HipAttnHandler.build_cos_sin(dim, shape.max_position, inv)
    if shape.rope_type != "yarn":
        raise ValueError(f"rope_type must be 'default' or 'yarn', not {shape.rope_type!r}")
    inv, factor = yarn_inv_freq(shape, device)
    return (HipAttnHandler.build_cos_sin(shape.rope_head_dim, shape.max_position, inv) * factor).contiguous()


def attention_sm_scale(shape: DeepseekV2Shape) -> float:
    """(nope + rope)^-0.5, times mscale(factor, mscale_all_dim)^2 under yarn (transformers' yarn_apply_mscale)"""
    scale = float(shape.nope_head_dim + shape.rope_head_dim) ** -0.5
    if shape.rope_type != "default" and shape.mscale_all_dim:
        m = _yarn_mscale(shape.rope_factor, shape.mscale_all_dim)
        scale = scale * m * m
    return scale


def check_supported(shape: DeepseekV2Shape, parallel_args: Optional[ParallelArgs], quant_method: str,
                    custom_allreduce=None) -> None:
    """everything DeepseekV2DecodeStep refuses, before it touches a GPU"""
    pa = parallel_args or ParallelArgs()
    if pa.world_size > 1 or custom_allreduce is not None:
        raise ValueError("DeepseekV2DecodeStep runs on one rank: tensor / expert parallelism is out of scope")
    if quant_method not in ("none", "fp8"):
        raise ValueError(f"quant_method must be 'none' or 'fp8', not {quant_method!r}")
    if shape.topk_method != "greedy":
        raise ValueError(f"topk_method {shape.topk_method!r} is not supported: group_limited_greedy scores a group by "
                         "its maximum, which the routing kernels do not offer; only 'greedy'")
    if shape.routed_scaling_factor != 1.0:
        raise ValueError("routed_scaling_factor other than 1 is not supported: folding it into the weights would "
                         "round them a second time")
    if shape.rope_type not in ("default", "yarn"):
        raise ValueError(f"rope_type must be 'default' or 'yarn', not {shape.rope_type!r}")


class DeepseekV2DecodeStep:
    def __init__(self, shape: DeepseekV2Shape, max_batch_tokens: int, n_blocks: int, block_size: int,
                 parallel_args: Optional[ParallelArgs] = None, quant_method: str = "none",
                 dtype=torch.bfloat16, device="cuda", seed: int = 0, custom_allreduce=None,
                 keep_checkpoint: bool = False, record_routing: bool = False):
        check_supported(shape, parallel_args, quant_method, custom_allreduce)
        pa = parallel_args or ParallelArgs()
        # keep_checkpoint: self.ckpt[layer] is the layer's state dict under the HuggingFace names relative to
        # model.layers.{i}. (self_attn.*, mlp.*), as the layers' load_state_dict took it
        self.ckpt = [] if keep_checkpoint else None
        self.shape, self.pa, self.dtype, self.device = shape, pa, dtype, torch.device(device)
        self.quant_method = quant_method
        self.defer_splitk = os.environ.get("SLM_DEFER_SPLITK", "1") != "0"  # read once, at build time
        self.block_size = block_size
        self._sample_bufs = None
        s, dev, T = shape, self.device, max_batch_tokens
        H, E, k = s.hidden, s.n_routed_experts, s.topk
        gen = torch.Generator(device=dev).manual_seed(seed * 1000 + 43)
        fp8 = quant_method == "fp8"
        qa = QuantArgs("fp8", 8) if fp8 else None
        Col, Row = (ColumnParallelFp8Linear, RowParallelFp8Linear) if fp8 else (ColumnParallelLinear, RowParallelLinear)
        draw = lambda n, kk: (torch.randn(n, kk, device=dev, generator=gen) * 0.02).to(dtype)  # noqa: E731
        norm_w = lambda n=H: (1 + 0.05 * torch.randn(n, device=dev, generator=gen)).to(dtype)  # noqa: E731

        def put(sd, name, n, kk):
            """one linear under `name` + ".weight" (fp8: e4m3 + ".weight_scale")"""
            w = draw(n, kk)
            if fp8:
                sd[name + ".weight"], sd[name + ".weight_scale"] = kernels.quantize_fp8_weight(w)
            else:
                sd[name + ".weight"] = w

        sub = lambda sd, p: {kk[len(p):]: v for kk, v in sd.items() if kk.startswith(p)}  # noqa: E731
        cos_sin = rope_cos_sin_table(s, dev)
        qk = s.nope_head_dim + s.rope_head_dim
        self.layers = []
        self.routing = [] if record_routing else None   # per SPARSE layer, in layer order
        self.sparse_layers = [li for li in range(s.n_layers) if li >= s.first_k_dense_replace]
        for li in range(s.n_layers):
            L, sd = {}, {}
            a = "self_attn."
            if s.q_lora_rank is None:
                put(sd, a + "q_proj", s.n_heads * qk, H)
            else:
                put(sd, a + "q_a_proj", s.q_lora_rank, H)
                sd[a + "q_a_layernorm.weight"] = norm_w(s.q_lora_rank)
                put(sd, a + "q_b_proj", s.n_heads * qk, s.q_lora_rank)
            put(sd, a + "kv_a_proj_with_mqa", s.kv_lora_rank + s.rope_head_dim, H)
            sd[a + "kv_a_layernorm.weight"] = norm_w(s.kv_lora_rank)
            put(sd, a + "kv_b_proj", s.n_heads * (s.nope_head_dim + s.v_head_dim), s.kv_lora_rank)
            put(sd, a + "o_proj", H, s.n_heads * s.v_head_dim)
            L["attn"] = MLAAttention(H, s.n_heads, s.nope_head_dim, s.rope_head_dim, s.v_head_dim, s.kv_lora_rank,
                                     s.q_lora_rank, cos_sin, True, attention_sm_scale(s), s.rms_eps, T,
                                     quant_method=quant_method, parallel_args=pa, dtype=dtype, device=dev)
            L["attn"].load_state_dict(sub(sd, a))
            L["attn"].verify_loaded_weights()
            sparse = li >= s.first_k_dense_replace
            m = "mlp.shared_experts." if sparse else "mlp."
            inter = s.n_shared_experts * s.moe_intermediate if sparse else s.intermediate
            for name, (n, kk) in (("gate_proj", (inter, H)), ("up_proj", (inter, H)), ("down_proj", (H, inter))):
                put(sd, m + name, n, kk)
            L["gate_up"] = Col(H, 2 * inter, False, False, pa, dtype, dev, act_mul="silu")
            L["gate_up"].load_state_dict(sub(sd, m), prefixes=["gate_proj.", "up_proj."])
            L["down"] = Row(inter, H, False, True, pa, dtype, dev)
            L["down"].load_state_dict(sub(sd, m + "down_proj."))
            for lin in (L["gate_up"], L["down"]):
                lin.verify_loaded_weights()
            L["inter"] = inter
            if sparse:
                sd["mlp.gate.weight"] = draw(E, H)
                for e in range(E):
                    for wn, hf, (n, kk) in (("w1", "gate_proj", (s.moe_intermediate, H)),
                                            ("w3", "up_proj", (s.moe_intermediate, H)),
                                            ("w2", "down_proj", (H, s.moe_intermediate))):
                        put(sd, f"mlp.experts.{e}.{hf}", n, kk)
                # FusedMoE takes the Mixtral names w1 | w3 | w2 for gate | up | down
                ren = {"gate_proj": "w1", "up_proj": "w3", "down_proj": "w2"}
                msd = {"gate.weight": sd["mlp.gate.weight"]}
                for kk, v in sub(sd, "mlp.experts.").items():
                    e, hf, rest = kk.split(".", 2)
                    msd[f"experts.{e}.{ren[hf]}.{rest}"] = v
                L["moe"] = FusedMoE(H, s.moe_intermediate, E, k, qa, scoring="softmax", renormalize=s.norm_topk_prob,
                                    max_tokens=T, dtype=dtype, device=dev, router="fused")
                L["moe"].load_state_dict(msd)
                L["moe"].experts.repack()
                if record_routing:
                    mb = L["moe"]._buffers()
                    self.routing.append(dict(logits=torch.zeros(T, E, dtype=torch.float32, device=dev),
                                             indices=mb["ids"].view(T, k), weights=mb["weights"].view(T, k)))
            L["in_norm"], L["post_norm"] = norm_w(), norm_w()
            sd["input_layernorm.weight"], sd["post_attention_layernorm.weight"] = L["in_norm"], L["post_norm"]
            L["kv"] = LatentKVCache(n_blocks, block_size, s.kv_lora_rank, s.rope_head_dim, dtype, dev)
            if keep_checkpoint:
                self.ckpt.append(sd)
            self.layers.append(L)
        self.final_norm = norm_w()
        self.embed = draw(s.vocab, H)
        self.lm_head = draw(H, s.vocab)
        e = lambda *sz: torch.empty(*sz, dtype=dtype, device=dev)  # noqa: E731
        # one SiLU * mul buffer per MLP width (the dense layers' and the shared experts')
        self.buf = dict(resid=e(T, H), normed=e(T, H), o=e(T, H), mlp=e(T, H), shared=e(T, H), moe=e(T, H),
                        act={w: e(T, w) for w in sorted({L["inter"] for L in self.layers})})

    def reserve_workspaces(self, n_tokens: int, max_kv_len: int) -> None:
        """Grow the kernel workspaces and build the per-token-count index lists once, before graph capture."""
        s = self.shape
        need = n_tokens * s.n_heads * 256 * (s.kv_lora_rank + 2) * 4   # worst-case split-KV partials
        need = max(need, 64 * n_tokens * s.hidden * 4)
        widest = max(s.hidden, s.n_heads * (s.nope_head_dim + s.rope_head_dim) + s.kv_lora_rank + s.rope_head_dim)
        kernels.reserve_workspace(min(need, 4 << 30), self.device, deferred_nbytes=16 * n_tokens * widest * 4)
        for L in self.layers:
            L["attn"].prepare(n_tokens)

    def _trunk(self, tokens: torch.Tensor, positions: torch.Tensor, params: InputParameters) -> torch.Tensor:
        """Embedding and the decoder stack: the final-norm output of all T rows (a view of the static buffer)."""
        s, b = self.shape, self.buf
        T = tokens.numel()
        eps, defer = s.rms_eps, self.defer_splitk
        resid, normed = b["resid"][:T], b["normed"][:T]
        resid.copy_(self.embed[tokens.long()])
        kernels.rms_norm(normed, resid, self.layers[0]["in_norm"], eps)
        sparse_i = 0
        for li, L in enumerate(self.layers):
            o = L["attn"].forward(normed, positions, L["kv"], params, out=b["o"][:T], defer_splitk=defer)
            # resid += o (from its slabs); normed = RMSNorm(resid) * post_norm
            kernels.rms_norm(normed, o, L["post_norm"], eps, residual=resid,
                             partials=L["attn"].o.deferred if defer else None)
            nxt = self.layers[li + 1]["in_norm"] if li + 1 < len(self.layers) else self.final_norm
            act = L["gate_up"].forward(normed, out=b["act"][L["inter"]][:T])
            if "moe" not in L:
                y = L["down"].forward(act, out=b["mlp"][:T], reduce=False, defer_splitk=defer)
                kernels.rms_norm(normed, y, nxt, eps, residual=resid, partials=L["down"].deferred if defer else None)
                continue
            shared = L["down"].forward(act, out=b["shared"][:T], reduce=False)
            logits_out = self.routing[sparse_i]["logits"][:T] if self.routing is not None else None
            sparse_i += 1
            y = L["moe"].forward(normed, out=b["moe"][:T], router_logits_out=logits_out, shared_out=shared)
            kernels.rms_norm(normed, y, nxt, eps, residual=resid)
        return normed

    def forward(self, tokens: torch.Tensor, positions: torch.Tensor, params: InputParameters,
                return_logits: bool = False, sampling=None):
        """tokens / positions [T] int32 -> next-token ids [n_seqs] (greedy) of each sequence's last token, or the
        logits [n_seqs, vocab] (return_logits), or a sampling.SampleOutput over static buffers (sampling:
        sampling.SamplingParameters with >= n_seqs rows; the RNG position of a sequence is the position of its last
        input token).  With record_routing, self.routing[i]["logits" | "indices" | "weights"][:T] hold the router's
        outputs of sparse layer self.sparse_layers[i] afterwards."""
        if sampling is not None and return_logits:
            raise ValueError("forward(): return_logits and sampling exclude each other")
        normed = self._trunk(tokens, positions, params)
        last = (params.q_cu_seq_lens[1:] - 1).long()
        self.last_hidden = normed[last]
        logits = self.last_hidden @ self.lm_head   # plain library GEMM, as the Llama step's
        if sampling is not None:
            return self._sample(logits, positions[last], sampling)
        if return_logits:
            return logits
        return torch.argmax(logits, dim=-1).to(torch.int32)

    def _sample(self, logits: torch.Tensor, last_positions: torch.Tensor, sampling):
        """The fused sampling kernel over the logits into static output buffers (LlamaDecodeStep._sample)."""
        from ._lib import SLM_SAMPLE_MAX_TOP
        from .sampling import SampleOutput, sample_logits
        n = logits.size(0)
        T = self.buf["resid"].size(0)
        if self._sample_bufs is None:
            e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=self.device)  # noqa: E731
            self._sample_bufs = dict(tok=e(T, dt=torch.int32), lp=e(T), top_lp=e(T * SLM_SAMPLE_MAX_TOP),
                                     top_tok=e(T * SLM_SAMPLE_MAX_TOP, dt=torch.int32))
        b, k = self._sample_bufs, sampling.max_top_logprobs
        out = SampleOutput(b["tok"][:n], None, b["lp"][:n] if sampling.logprobs else None,
                           b["top_lp"][:n * k].view(n, k) if sampling.logprobs and k else None,
                           b["top_tok"][:n * k].view(n, k) if sampling.logprobs and k else None)
        return sample_logits(logits, sampling.narrow(n), last_positions, out=out)
