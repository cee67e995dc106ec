"""A Mixtral-shaped decode step on the fused path, beside decode.LlamaDecodeStep and gemma2.Gemma2DecodeStep and on
their contract: seeded synthetic checkpoint (keep_checkpoint), static buffers, forward(tokens, positions, params,
return_logits, sampling), capturable with torch.cuda.graph on one stream, one lane, one rank.  It is the Llama step
with the dense MLP replaced by a sparse mixture of experts (HuggingFace MixtralDecoderLayer):

  embedding -> the first input norm                                             kernels.rms_norm
  per layer
    qkv GEMM (split-K slabs deferred) -> RoPE + KV append                       Attention.append
    paged attention                                                              Attention.decode
    o GEMM (deferred) -> residual + post-attention norm                          kernels.rms_norm(residual=, partials=)
    router: gate GEMM + top-k softmax, renormalised, ONE launch                  kernels.moe_router
      -> block alignment -> grouped gate_up GEMM, SiLU * mul -> grouped down GEMM, routing weight on the
         accumulator -> sum over a token's experts                               moe.FusedMoE(router="fused")
    residual + the next layer's input norm (or the final norm)                   kernels.rms_norm(residual=)
  untied lm_head, no cap -> argmax, or the fused sampling kernel

quant_method "none" (f16 / bf16 checkpoint), "fp8" (e4m3 weights with channel scales, W8A16), "mxfp4" (OCP MXFP4:
e2m1 nibbles + e8m0 block scales, W4A16, the "none" checkpoint of the same seed quantised, loaded under the Quark
names weight / weight_scale) or "awq" (int4): the four attention linears are the classes LlamaDecodeStep uses for
that method, the experts the matching experts class of moe.py, loaded through load_state_dict under the Mixtral names
experts.{e}.w1|w2|w3.*; gate.weight, the embedding, the head and the norms stay in T.

Out of scope: tensor- or expert-parallel Mixtral (world_size > 1 is refused), two lanes, a C++ host step.
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
class MixtralShape:
    hidden: int = 4096
    n_heads: int = 32
    n_kv_heads: int = 8
    head_dim: int = 128
    intermediate: int = 14336
    n_layers: int = 32
    vocab: int = 32000
    rope_theta: float = 1e6
    rms_eps: float = 1e-5
    max_position: int = 131072
    n_experts: int = 8
    topk: int = 2

    @staticmethod
    def mixtral_8x7b() -> "MixtralShape":
        """the defaults of transformers.MixtralConfig() (tests/test_moe_router_cpu.py compares field by field)"""
        return MixtralShape()

    @staticmethod
    def mixtral_8x22b() -> "MixtralShape":
        """UNVERIFIED: written from memory of the public mistralai/Mixtral-8x22B-v0.1 config.json, which was not
        at hand to check against; compare with the checkpoint's own config before relying on it"""
        return MixtralShape(hidden=6144, n_heads=48, n_kv_heads=8, head_dim=128, intermediate=16384, n_layers=56,
                            max_position=65536)

    @staticmethod
    def tiny() -> "MixtralShape":
        """the int4 (K % 128, N % 64) and the dense / fp8 (% 32) grouped GEMMs all accept these sizes"""
        return MixtralShape(hidden=256, n_heads=8, n_kv_heads=2, head_dim=32, intermediate=512, n_layers=2,
                            vocab=1024, max_position=512, n_experts=8, topk=2)


class MixtralDecodeStep:
    def __init__(self, shape: MixtralShape, max_batch_tokens: int, n_blocks: int, block_size: int,
                 parallel_args: Optional[ParallelArgs] = None, quant_method: str = "none", group_size: int = 128,
                 dtype=torch.bfloat16, device="cuda", seed: int = 0, custom_allreduce=None,
                 keep_checkpoint: bool = False, record_routing: bool = False):
        pa = parallel_args or ParallelArgs()
        if pa.world_size > 1 or custom_allreduce is not None:
            raise ValueError("MixtralDecodeStep runs on one rank: tensor-parallel sharding of an expert is out of scope")
        if quant_method not in ("none", "fp8", "awq", "mxfp4"):
            raise ValueError(f"quant_method must be 'none', 'fp8', 'awq' or 'mxfp4', not {quant_method!r}")
        # keep_checkpoint: retain the CHECKPOINT-format tensors (self.ckpt[layer]: "qkv", "o" as the linears take
        # them, "moe" the state dict FusedMoE.load_state_dict took) so a parity test can rebuild the model on the CPU
        self.ckpt = [] if keep_checkpoint else None
        self.shape, self.pa, self.dtype, self.device = shape, pa, dtype, torch.device(device)
        self.quant_method, self.group_size = quant_method, group_size
        self.defer_splitk = os.environ.get("SLM_DEFER_SPLITK", "1") != "0"  # read once, at build time
        self.block_size = block_size
        self.n_heads, self.n_kv_heads = shape.n_heads, shape.n_kv_heads
        self._sample_bufs = None
        D, H, inter, E, k = shape.head_dim, shape.hidden, shape.intermediate, shape.n_experts, shape.topk
        dev, T = self.device, max_batch_tokens
        gen = torch.Generator(device=dev).manual_seed(seed * 1000 + 41)
        inv_freq = 1.0 / (shape.rope_theta ** (torch.arange(0, D, 2, dtype=torch.float32, device=dev) / D))
        cos_sin = HipAttnHandler.build_cos_sin(D, shape.max_position, inv_freq)
        handler = HipAttnHandler(sm_scale=D ** -0.5, rotary_dim=D, cos_sin=cos_sin, interleaved=False)
        self.attn = Attention(shape.n_heads, shape.n_kv_heads, D, handler)
        nq, nkv = shape.n_heads * D, shape.n_kv_heads * D
        qa = {"none": None, "fp8": QuantArgs("fp8", 8), "mxfp4": QuantArgs("mxfp4", 4),
              "awq": QuantArgs(quant_method="awq", bits=4, group_size=group_size, zero_point=True)}[quant_method]
        draw = lambda n, kk: (torch.randn(n, kk, device=dev, generator=gen) * 0.02).to(dtype)  # noqa: E731
        norm_w = lambda: (1 + 0.05 * torch.randn(H, device=dev, generator=gen)).to(dtype)  # noqa: E731
        self.layers = []
        # per layer (record_routing): the router's logits_out [T, E] and the layer's own indices / weights buffers
        self.routing = [] if record_routing else None
        for _ in range(shape.n_layers):
            L, ck = {}, {}
            for name, (K, N) in (("qkv", (H, nq + 2 * nkv)), ("o", (nq, H))):
                col = name == "qkv"
                if quant_method == "awq":
                    L[name] = ColumnParallelQLinear(K, N, False, qa, False, pa, dtype, dev) if col else \
                        RowParallelQLinear(K, N, False, qa, True, pa, dtype, dev)
                    ck[name] = _rand_int4_linear(gen, K, N, group_size, "awq", dtype, dev)
                    L[name].load_state_dict(ck[name])
                    L[name].verify_loaded_weights()
                    L[name]._repack()
                    continue
                Col, Row = (ColumnParallelFp8Linear, RowParallelFp8Linear) if quant_method == "fp8" else \
                    (ColumnParallelMxfp4Linear, RowParallelMxfp4Linear) if quant_method == "mxfp4" else \
                    (ColumnParallelLinear, RowParallelLinear)
                L[name] = Col(K, N, False, False, pa, dtype, dev) if col else Row(K, N, False, True, pa, dtype, dev)
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
            L["moe"] = FusedMoE(H, inter, E, k, qa, scoring="softmax", renormalize=True, max_tokens=T, dtype=dtype,
                                device=dev, router="fused")
            L["moe"].load_state_dict(sd)
            L["moe"].experts.repack()
            ck["moe"] = sd
            if keep_checkpoint:
                self.ckpt.append(ck)
            L["in_norm"], L["post_norm"] = norm_w(), norm_w()
            L["kv"] = KVCache(n_blocks, block_size, shape.n_kv_heads, D, dtype, dev)
            if record_routing:
                mb = L["moe"]._buffers()
                self.routing.append(dict(logits=torch.zeros(T, E, dtype=torch.float32, device=dev),
                                         indices=mb["ids"].view(T, k), weights=mb["weights"].view(T, k)))
            self.layers.append(L)
        self.final_norm = norm_w()
        self.embed = draw(shape.vocab, H)
        self.lm_head = draw(H, shape.vocab)
        e = lambda *s: torch.empty(*s, dtype=dtype, device=dev)  # noqa: E731
        self.buf = dict(resid=e(T, H), normed=e(T, H), qkv=e(T, nq + 2 * nkv), attn=e(T, shape.n_heads, D),
                        o=e(T, H), moe=e(T, H))

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
        resid, normed, moe_out = b["resid"][:T], b["normed"][:T], b["moe"][:T]
        resid.copy_(self.embed[tokens.long()])
        kernels.rms_norm(normed, resid, self.layers[0]["in_norm"], eps)
        for li, L in enumerate(self.layers):
            qkv = L["qkv"].forward(normed, out=b["qkv"][:T], defer_splitk=defer)
            q = self.attn.append(qkv[:, :nq], qkv[:, nq:nq + nkv], qkv[:, nq + nkv:], positions, L["kv"], params,
                                 qkv_partials=L["qkv"].deferred if defer else None)
            attn = self.attn.decode(q, L["kv"], params, output=b["attn"][:T])
            o = L["o"].forward(attn, out=b["o"][:T], reduce=False, defer_splitk=defer)
            # resid += o (from its slabs); normed = RMSNorm(resid) * post_norm
            kernels.rms_norm(normed, o, L["post_norm"], eps, residual=resid,
                             partials=L["o"].deferred if defer else None)
            L["moe"].forward(normed, out=moe_out,
                             router_logits_out=self.routing[li]["logits"][:T] if self.routing is not None else None)
            nxt = self.layers[li + 1]["in_norm"] if li + 1 < len(self.layers) else self.final_norm
            kernels.rms_norm(normed, moe_out, nxt, eps, residual=resid)
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
