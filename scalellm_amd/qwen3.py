"""Qwen3- and Qwen3-MoE-shaped decode steps on the fused path, beside mixtral.MixtralDecodeStep and on its contract:
seeded synthetic checkpoint (keep_checkpoint), static buffers, forward(tokens, positions, params, return_logits,
sampling), capturable with torch.cuda.graph on one stream, one lane, one rank.  It is the Llama step with Qwen3's
per-head RMSNorm of q and k before RoPE (HuggingFace Qwen3Attention: q_norm, k_norm, [head_dim] weights shared by the
heads, eps = rms_norm_eps), and with n_experts > 0 the MLP replaced by Qwen3-MoE's sparse block:

  embedding -> the first input norm                                             kernels.rms_norm
  per layer
    qkv GEMM (split-K slabs deferred) -> per-head q / k norm + RoPE + KV append kernels.qk_norm_rope_kv_append
    paged attention                                                              Attention.decode
    o GEMM (deferred) -> residual + post-attention norm                          kernels.rms_norm(residual=, partials=)
    n_experts == 0: gate_up GEMM with the SiLU * mul epilogue -> down GEMM (deferred)
    n_experts  > 0: router (softmax, top-k, renormalised when norm_topk_prob) -> grouped expert GEMMs
                                                                                 moe.FusedMoE(router="fused")
    residual + the next layer's input norm (or the final norm)                   kernels.rms_norm(residual=)
  lm_head (the embedding itself when tie_word_embeddings) -> argmax, or the fused sampling kernel

quant_method "none" (f16 / bf16 checkpoint), "fp8" (e4m3 weights with channel scales, W8A16), "mxfp4" (OCP MXFP4,
W4A16: the attention projections and the dense MLP on layers.{Column,Row}ParallelMxfp4Linear, the experts on
moe.MoEMxfp4Experts) or "awq" (int4), as MixtralDecodeStep.  head_dim must be one the QK-norm kernel takes (64, 128, 256).

Out of scope, refused: world_size > 1, a custom all-reduce.  Not offered: two lanes, a C++ host step,
mlp_only_layers / decoder_sparse_step (with n_experts > 0 every layer is sparse), sliding-window layers, Gemma-3's
(1 + w) QK-norm.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import kernels
from .decode import _rand_int4_linear
from .layers import (Attention, ColumnParallelFp8Linear, ColumnParallelLinear, ColumnParallelMxfp4Linear,
                     ColumnParallelQLinear, HipAttnHandler, InputParameters, KVCache, QuantArgs, RowParallelFp8Linear,
                     RowParallelLinear, RowParallelMxfp4Linear, RowParallelQLinear)
from .model_parallel import ParallelArgs
from .moe import FusedMoE


@dataclass
class Qwen3Shape:
    hidden: int = 4096
    n_heads: int = 32
    n_kv_heads: int = 8
    head_dim: int = 128               # a field of its own: n_heads * head_dim != hidden in Qwen3-0.6B
    intermediate: int = 12288
    n_layers: int = 36
    vocab: int = 151936
    rope_theta: float = 1e6
    rms_eps: float = 1e-6
    max_position: int = 40960
    tie_word_embeddings: bool = False
    n_experts: int = 0                # 0: the dense Qwen3 MLP
    topk: int = 0
    moe_intermediate: int = 0
    norm_topk_prob: bool = True

    @staticmethod
    def qwen3_8b() -> "Qwen3Shape":
        """UNVERIFIED: written from memory of the public Qwen/Qwen3-8B config.json, which was not at hand to check
        against; compare with the checkpoint's own config before relying on it"""
        return Qwen3Shape()

    @staticmethod
    def qwen3_30b_a3b() -> "Qwen3Shape":
        """UNVERIFIED: written from memory of the public Qwen/Qwen3-30B-A3B config.json, which was not at hand to
        check against; compare with the checkpoint's own config before relying on it"""
        return Qwen3Shape(hidden=2048, n_heads=32, n_kv_heads=4, head_dim=128, intermediate=6144, n_layers=48,
                          n_experts=128, topk=8, moe_intermediate=768, norm_topk_prob=True)

    @staticmethod
    def tiny() -> "Qwen3Shape":
        """the int4 (K % 128, N % 64) and the dense / fp8 (% 32) GEMMs all accept these sizes; n_heads * head_dim =
        512 != hidden, as in Qwen3-0.6B"""
        return Qwen3Shape(hidden=256, n_heads=8, n_kv_heads=2, head_dim=64, intermediate=512, n_layers=2, vocab=1024,
                          max_position=512)

    @staticmethod
    def tiny_moe() -> "Qwen3Shape":
        """tiny() with 8 experts, top 2, expert intermediate 128 (the grouped GEMMs' limits, int4 included)"""
        return Qwen3Shape(hidden=256, n_heads=8, n_kv_heads=2, head_dim=64, intermediate=512, n_layers=2, vocab=1024,
                          max_position=512, n_experts=8, topk=2, moe_intermediate=128, norm_topk_prob=True)


class Qwen3DecodeStep:
    def __init__(self, shape: Qwen3Shape, max_batch_tokens: int, n_blocks: int, block_size: int,
                 parallel_args: Optional[ParallelArgs] = None, quant_method: str = "none", group_size: int = 128,
                 dtype=torch.bfloat16, device="cuda", seed: int = 0, custom_allreduce=None,
                 keep_checkpoint: bool = False, record_routing: bool = False):
        pa = parallel_args or ParallelArgs()
        if pa.world_size > 1 or custom_allreduce is not None:
            raise ValueError("Qwen3DecodeStep runs on one rank: tensor parallelism is out of scope")
        if quant_method not in ("none", "fp8", "awq", "mxfp4"):
            raise ValueError(f"quant_method must be 'none', 'fp8', 'awq' or 'mxfp4', not {quant_method!r}")
        if shape.head_dim not in (64, 128, 256):
            raise ValueError(f"head_dim {shape.head_dim}: the QK-norm prologue takes 64, 128 or 256")
        if record_routing and not shape.n_experts:
            raise ValueError("record_routing needs a mixture-of-experts shape")
        # keep_checkpoint: retain the CHECKPOINT-format tensors (self.ckpt[layer]: "qkv", "o", and "gate_up" /
        # "down" or "moe" (the state dict FusedMoE.load_state_dict took)) so a parity test can rebuild the model
        self.ckpt = [] if keep_checkpoint else None
        self.shape, self.pa, self.dtype, self.device = shape, pa, dtype, torch.device(device)
        self.quant_method, self.group_size = quant_method, group_size
        self.defer_splitk = os.environ.get("SLM_DEFER_SPLITK", "1") != "0"  # read once, at build time
        self.block_size = block_size
        self.n_heads, self.n_kv_heads = shape.n_heads, shape.n_kv_heads
        self._sample_bufs = None
        D, H, E, k = shape.head_dim, shape.hidden, shape.n_experts, shape.topk
        inter = shape.moe_intermediate if E else shape.intermediate
        dev, T = self.device, max_batch_tokens
        gen = torch.Generator(device=dev).manual_seed(seed * 1000 + 43)
        inv_freq = 1.0 / (shape.rope_theta ** (torch.arange(0, D, 2, dtype=torch.float32, device=dev) / D))
        self.cos_sin = HipAttnHandler.build_cos_sin(D, shape.max_position, inv_freq)
        nq, nkv = shape.n_heads * D, shape.n_kv_heads * D
        qa = {"none": None, "fp8": QuantArgs("fp8", 8), "mxfp4": QuantArgs("mxfp4", 4),
              "awq": QuantArgs(quant_method="awq", bits=4, group_size=group_size, zero_point=True)}[quant_method]
        draw = lambda n, kk: (torch.randn(n, kk, device=dev, generator=gen) * 0.02).to(dtype)  # noqa: E731
        norm_w = lambda n=H: (1 + 0.05 * torch.randn(n, device=dev, generator=gen)).to(dtype)  # noqa: E731
        linears = [("qkv", (H, nq + 2 * nkv)), ("o", (nq, H))]
        if not E:
            linears += [("gate_up", (H, 2 * inter)), ("down", (inter, H))]
        self.layers = []
        # per layer (record_routing): the router's logits_out [T, E] and the layer's own indices / weights buffers
        self.routing = [] if record_routing else None
        for _ in range(shape.n_layers):
            L, ck = {}, {}
            for name, (K, N) in linears:
                col = name in ("qkv", "gate_up")
                act = "silu" if name == "gate_up" else None
                if quant_method == "awq":
                    L[name] = ColumnParallelQLinear(K, N, False, qa, False, pa, dtype, dev, act_mul=act) if col else \
                        RowParallelQLinear(K, N, False, qa, True, pa, dtype, dev)
                    ck[name] = _rand_int4_linear(gen, K, N, group_size, "awq", dtype, dev)
                    L[name].load_state_dict(ck[name])
                    L[name].verify_loaded_weights()
                    L[name]._repack()
                    continue
                Col, Row = (ColumnParallelFp8Linear, RowParallelFp8Linear) if quant_method == "fp8" else \
                    (ColumnParallelMxfp4Linear, RowParallelMxfp4Linear) if quant_method == "mxfp4" else \
                    (ColumnParallelLinear, RowParallelLinear)
                L[name] = Col(K, N, False, False, pa, dtype, dev, act_mul=act) if col else \
                    Row(K, N, False, True, pa, dtype, dev)
                w = draw(N, K)
                if quant_method == "fp8":
                    w8, sc = kernels.quantize_fp8_weight(w)
                    ck[name] = {"weight": w8, "weight_scale": sc}
                    L[name].load_shard(w8, sc)
                elif quant_method == "mxfp4":   # the same checkpoint quantised to MXFP4, under the Quark names
                    w4, sc = kernels.quantize_mxfp4_weight(w)
                    ck[name] = {"weight": w4, "weight_scale": sc}
                    L[name].load_state_dict(ck[name])
                else:
                    ck[name] = {"weight": w}
                    L[name].load_shard(w)
                L[name].verify_loaded_weights()
            if E:
                sd = {"gate.weight": draw(E, H)}
                for e in range(E):
                    for wn, (N, K) in (("w1", (inter, H)), ("w3", (inter, H)), ("w2", (H, inter))):
                        p = f"experts.{e}.{wn}."
                        if quant_method == "awq":
                            for tn, t in _rand_int4_linear(gen, K, N, group_size, "awq", dtype, dev).items():
                                sd[p + tn] = t
                        elif quant_method == "fp8":
                            sd[p + "weight"], sd[p + "weight_scale"] = kernels.quantize_fp8_weight(draw(N, K))
                        elif quant_method == "mxfp4":
                            sd[p + "weight"], sd[p + "weight_scale"] = kernels.quantize_mxfp4_weight(draw(N, K))
                        else:
                            sd[p + "weight"] = draw(N, K)
                L["moe"] = FusedMoE(H, inter, E, k, qa, scoring="softmax", renormalize=shape.norm_topk_prob,
                                    max_tokens=T, dtype=dtype, device=dev, router="fused")
                L["moe"].load_state_dict(sd)
                L["moe"].experts.repack()
                ck["moe"] = sd
            if keep_checkpoint:
                self.ckpt.append(ck)
            L["in_norm"], L["post_norm"] = norm_w(), norm_w()
            L["q_norm"], L["k_norm"] = norm_w(D), norm_w(D)
            handler = HipAttnHandler(sm_scale=D ** -0.5, rotary_dim=D, cos_sin=self.cos_sin, interleaved=False,
                                     q_norm=L["q_norm"], k_norm=L["k_norm"], qk_norm_eps=shape.rms_eps)
            L["attn"] = Attention(shape.n_heads, shape.n_kv_heads, D, handler)
            L["kv"] = KVCache(n_blocks, block_size, shape.n_kv_heads, D, dtype, dev)
            if record_routing:
                mb = L["moe"]._buffers()
                self.routing.append(dict(logits=torch.zeros(T, E, dtype=torch.float32, device=dev),
                                         indices=mb["ids"].view(T, k), weights=mb["weights"].view(T, k)))
            self.layers.append(L)
        self.final_norm = norm_w()
        self.embed = draw(shape.vocab, H)
        # tied: logits = h . embed^T (a view, no copy)
        self.lm_head = self.embed.t() if shape.tie_word_embeddings else draw(H, shape.vocab)
        e = lambda *s: torch.empty(*s, dtype=dtype, device=dev)  # noqa: E731
        self.buf = dict(resid=e(T, H), normed=e(T, H), qkv=e(T, nq + 2 * nkv), attn=e(T, shape.n_heads, D),
                        o=e(T, H), mlp=e(T, H))
        if not E:
            self.buf["act"] = e(T, inter)

    def set_qk_norm_fused(self, fused: bool) -> None:
        """False: every layer runs the QK-norm prologue as the composition of the older entry points (the qkv GEMM
        then reduces its own split-K slabs) -- the control the fused kernel is compared with"""
        for L in self.layers:
            L["attn"].handler.qk_norm_fused = fused

    def reserve_workspaces(self, n_tokens: int, max_kv_len: int) -> None:
        """Grow the kernel workspaces once, before graph capture."""
        s = self.shape
        need = n_tokens * s.n_heads * 256 * (s.head_dim + 2) * 4   # worst-case split-KV partials
        need = max(need, 64 * n_tokens * s.hidden * 4)
        widest = max(s.hidden, (s.n_heads + 2 * s.n_kv_heads) * s.head_dim)
        kernels.reserve_workspace(min(need, 4 << 30), self.device, deferred_nbytes=16 * n_tokens * widest * 4)

    def _trunk(self, tokens: torch.Tensor, positions: torch.Tensor, params: InputParameters) -> torch.Tensor:
        """Embedding and the decoder stack: the final-norm output of all T rows (a view of the static buffer)."""
        s, b = self.shape, self.buf
        T = tokens.numel()
        D, eps, defer = s.head_dim, s.rms_eps, self.defer_splitk
        nq, nkv = s.n_heads * D, s.n_kv_heads * D
        resid, normed, mlp_out = b["resid"][:T], b["normed"][:T], b["mlp"][:T]
        resid.copy_(self.embed[tokens.long()])
        kernels.rms_norm(normed, resid, self.layers[0]["in_norm"], eps)
        for li, L in enumerate(self.layers):
            attn_l = L["attn"]
            defer_qkv = defer and attn_l.handler.qk_norm_fused
            qkv = L["qkv"].forward(normed, out=b["qkv"][:T], defer_splitk=defer_qkv)
            q = attn_l.append(qkv[:, :nq], qkv[:, nq:nq + nkv], qkv[:, nq + nkv:], positions, L["kv"], params,
                              qkv_partials=L["qkv"].deferred if defer_qkv else None)
            attn = attn_l.decode(q, L["kv"], params, output=b["attn"][:T])
            o = L["o"].forward(attn, out=b["o"][:T], reduce=False, defer_splitk=defer)
            # resid += o (from its slabs); normed = RMSNorm(resid) * post_norm
            kernels.rms_norm(normed, o, L["post_norm"], eps, residual=resid,
                             partials=L["o"].deferred if defer else None)
            partials = None
            if s.n_experts:
                L["moe"].forward(normed, out=mlp_out,
                                 router_logits_out=self.routing[li]["logits"][:T] if self.routing is not None else None)
            else:
                act = L["gate_up"].forward(normed, out=b["act"][:T])   # silu(gate) * up in the GEMM epilogue
                L["down"].forward(act, out=mlp_out, reduce=False, defer_splitk=defer)
                partials = L["down"].deferred if defer else None
            nxt = self.layers[li + 1]["in_norm"] if li + 1 < len(self.layers) else self.final_norm
            kernels.rms_norm(normed, mlp_out, nxt, eps, residual=resid, partials=partials)
        return normed

    def forward(self, tokens: torch.Tensor, positions: torch.Tensor, params: InputParameters,
                return_logits: bool = False, sampling=None):
        """tokens / positions [T] int32 -> next-token ids [n_seqs] (greedy) of each sequence's last token, or the
        logits [n_seqs, vocab] (return_logits), or a sampling.SampleOutput over static buffers (sampling:
        sampling.SamplingParameters with >= n_seqs rows; the RNG position of a sequence is the position of its last
        input token).  With record_routing, self.routing[layer]["logits" | "indices" | "weights"][:T] hold the
        router's outputs of this step afterwards."""
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
