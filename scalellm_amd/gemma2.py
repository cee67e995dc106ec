"""A Gemma-2-shaped decode step on the fused path, beside decode.LlamaDecodeStep and on its contract: seeded synthetic
checkpoint (keep_checkpoint; int4 with quant_method "awq" / "gptq", f16 / bf16 with "none", which load_state_dict
replaces by a HuggingFace one), static buffers, forward(tokens, positions, params, return_logits, sampling),
capturable with torch.cuda.graph on one stream and one lane.  It drives the hot path the way the reference's
Gemma2ModelImpl::forward does (src/models/google/gemma2.h:186-204, 221-276, 298-343):

  embedding * T(sqrt(hidden)) + the first input norm            kernels.gemma_embed_norm   (form C)
  per layer
    qkv GEMM (split-K slabs deferred) -> RoPE + KV append       Attention.append
    paged attention: sm_scale = attn_scalar^-0.5, logit soft cap, sliding window on EVEN layers (gemma2.h:249-251)
    o GEMM (deferred) -> post_attention norm + residual + pre_feedforward norm   kernels.gemma_sandwich_norm (form B)
    gate_up GEMM -> gelu_new * up  (the polynomial of gelu_pytorch_tanh)         kernels.gelu_new_with_mul
    down GEMM (deferred) -> post_feedforward norm + residual + the next layer's input norm (or the final norm)
  lm_head on the tied embedding -> tanh(logits / cap) * cap     kernels.soft_cap
  argmax, or the fused sampling kernel

As many launches per layer as the Llama step has without its SiLU epilogue, plus one.  Single rank: the fused
all-reduce + RMSNorm of the tensor-parallel Llama step is Llama-normed.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import kernels
from .decode import _rand_int4_linear
from .layers import (Attention, ColumnParallelLinear, ColumnParallelQLinear, HipAttnHandler, InputParameters, KVCache,
                     QuantArgs, RowParallelLinear, RowParallelQLinear)
from .model_parallel import ParallelArgs


@dataclass
class Gemma2Shape:
    hidden: int = 2304
    n_heads: int = 8
    n_kv_heads: int = 4
    head_dim: int = 256
    intermediate: int = 9216
    n_layers: int = 26
    vocab: int = 256000
    rope_theta: float = 10000.0
    rms_eps: float = 1e-6
    max_position: int = 8192
    attn_scalar: float = 256.0              # query_pre_attn_scalar: sm_scale = attn_scalar ** -0.5
    sliding_window: int = 4096              # even layers; odd layers attend globally (gemma2.h:249-251)
    attn_logit_soft_cap: float = 50.0
    final_logit_soft_cap: float = 30.0

    @staticmethod
    def from_hf_config(cfg) -> "Gemma2Shape":
        """The shape of a HuggingFace Gemma2Config (the object, or the dict of its config.json).  HuggingFace's
        sliding_window counts the keys a query sees, itself included; the field here is the attention kernel's
        and counts the keys BEHIND the query (layers.Attention), so it is one less."""
        get = cfg.get if isinstance(cfg, dict) else lambda k, d=None: getattr(cfg, k, d)  # noqa: E731
        window = get("sliding_window")
        return Gemma2Shape(
            hidden=get("hidden_size"), n_heads=get("num_attention_heads"), n_kv_heads=get("num_key_value_heads"),
            head_dim=get("head_dim"), intermediate=get("intermediate_size"), n_layers=get("num_hidden_layers"),
            vocab=get("vocab_size"), rope_theta=float(get("rope_theta", 10000.0)),
            rms_eps=float(get("rms_norm_eps", 1e-6)), max_position=get("max_position_embeddings", 8192),
            attn_scalar=float(get("query_pre_attn_scalar")),
            sliding_window=int(window) - 1 if window and window > 0 else -1,
            attn_logit_soft_cap=float(get("attn_logit_softcapping") or 0.0),
            final_logit_soft_cap=float(get("final_logit_softcapping") or 0.0))

    # the public HuggingFace configs (google/gemma-2-{2b,9b,27b}/config.json)
    @staticmethod
    def gemma2_2b() -> "Gemma2Shape":
        return Gemma2Shape()

    @staticmethod
    def gemma2_9b() -> "Gemma2Shape":
        return Gemma2Shape(hidden=3584, n_heads=16, n_kv_heads=8, head_dim=256, intermediate=14336, n_layers=42)

    @staticmethod
    def gemma2_27b() -> "Gemma2Shape":
        return Gemma2Shape(hidden=4608, n_heads=32, n_kv_heads=16, head_dim=128, intermediate=36864, n_layers=46,
                           attn_scalar=144.0)


class Gemma2DecodeStep:
    def __init__(self, shape: Gemma2Shape, max_batch_tokens: int, n_blocks: int, block_size: int,
                 parallel_args: Optional[ParallelArgs] = None, quant_method: str = "awq", group_size: int = 128,
                 dtype=torch.bfloat16, device="cuda", seed: int = 0, custom_allreduce=None,
                 keep_checkpoint: bool = False):
        pa = parallel_args or ParallelArgs()
        if pa.world_size > 1 or custom_allreduce is not None:
            raise ValueError("Gemma2DecodeStep runs on one rank: the fused all-reduce + RMSNorm is Llama-normed")
        if shape.final_logit_soft_cap <= 0:
            raise ValueError("final_logit_soft_cap must be positive (gemma2.h:305)")
        # keep_checkpoint: retain the CHECKPOINT-format tensors (self.ckpt[layer][name]) so a parity test can
        # rebuild the same model on the CPU
        self.ckpt = [] if keep_checkpoint else None
        self.shape, self.pa, self.dtype, self.device = shape, pa, dtype, torch.device(device)
        self.defer_splitk = os.environ.get("SLM_DEFER_SPLITK", "1") != "0"  # read once, at build time
        self.block_size = block_size
        self.n_heads, self.n_kv_heads = shape.n_heads, shape.n_kv_heads
        self._sample_bufs = None
        D, H, inter = shape.head_dim, shape.hidden, shape.intermediate
        gen = torch.Generator(device=self.device).manual_seed(seed * 1000 + 29)
        # quant_method "none": an f16 / bf16 checkpoint ([out, in] weights, streamed as they are by the dense GEMM)
        self.quant_method = quant_method
        dense = quant_method == "none"
        qa = None if dense else \
            QuantArgs(quant_method=quant_method, bits=4, group_size=group_size, zero_point=(quant_method == "awq"))
        inv_freq = 1.0 / (shape.rope_theta ** (torch.arange(0, D, 2, dtype=torch.float32, device=self.device) / D))
        cos_sin = HipAttnHandler.build_cos_sin(D, shape.max_position, inv_freq)
        # ONE handler (scale, cap, rotary table) shared by every layer; the window is the layer's
        handler = HipAttnHandler(sm_scale=float(shape.attn_scalar) ** -0.5, logits_soft_cap=shape.attn_logit_soft_cap,
                                 rotary_dim=D, cos_sin=cos_sin, interleaved=False)
        nq, nkv = shape.n_heads * D, shape.n_kv_heads * D
        norm_w = lambda: (0.3 * torch.randn(H, device=self.device, generator=gen)).to(dtype)  # noqa: E731
        self.layers = []
        for li in range(shape.n_layers):
            L = {"attn": Attention(shape.n_heads, shape.n_kv_heads, D, handler,
                                   sliding_window=shape.sliding_window if li % 2 == 0 else -1)}
            ck = {}
            for name, (K, N) in (("qkv", (H, nq + 2 * nkv)), ("o", (nq, H)), ("gate_up", (H, 2 * inter)),
                                 ("down", (inter, H))):
                col = name in ("qkv", "gate_up")
                if dense:
                    L[name] = ColumnParallelLinear(K, N, False, False, pa, dtype, self.device) if col else \
                        RowParallelLinear(K, N, False, True, pa, dtype, self.device)
                    # unit-variance outputs for unit-variance inputs: the scores reach the soft cap's curved part
                    ck[name] = {"weight": (torch.randn(N, K, device=self.device, generator=gen) * K ** -0.5).to(dtype)}
                    L[name].load_shard(ck[name]["weight"])
                    L[name].verify_loaded_weights()
                    continue
                L[name] = ColumnParallelQLinear(K, N, False, qa, False, pa, dtype, self.device) if col else \
                    RowParallelQLinear(K, N, False, qa, True, pa, dtype, self.device)
                ck[name] = _rand_int4_linear(gen, K, N, group_size, quant_method, dtype, self.device)
                L[name].load_state_dict(ck[name])
                L[name].verify_loaded_weights()
                L[name]._repack()
            if keep_checkpoint:
                self.ckpt.append(ck)
            for name in ("in_norm", "post_attn_norm", "pre_ffn_norm", "post_ffn_norm"):
                L[name] = norm_w()   # checkpoint values: the kernel applies 1 + w
            L["kv"] = KVCache(n_blocks, block_size, shape.n_kv_heads, D, dtype, self.device)
            self.layers.append(L)
        self.final_norm = norm_w()
        # the lm_head is the embedding (gemma2.h:311: registered as "model.embed_tokens")
        self.embed = (torch.randn(shape.vocab, H, device=self.device, generator=gen) * 0.02).to(dtype)
        self.embed_scale = float(torch.tensor(float(H) ** 0.5, dtype=dtype).float())  # T(sqrt(hidden)), gemma2.h:236
        T = max_batch_tokens
        e = lambda *s: torch.empty(*s, dtype=dtype, device=self.device)  # noqa: E731
        self.buf = dict(resid=e(T, H), normed=e(T, H), qkv=e(T, nq + 2 * nkv), attn=e(T, shape.n_heads, D),
                        o=e(T, H), gate_up=e(T, 2 * inter), act=e(T, inter), down=e(T, H))

    def load_state_dict(self, sd) -> None:
        """Replace the synthetic checkpoint by the tensors of a HuggingFace Gemma2ForCausalLM state dict
        (quant_method "none"): q | k | v and gate | up are merged row-wise, as the fused GEMMs read them; the norm
        weights stay the checkpoint's w of (1 + w); the lm_head is the embedding."""
        if self.quant_method != "none":
            raise ValueError("load_state_dict takes an unquantised checkpoint: build the step with quant_method='none'")
        t = lambda name: sd[name].to(device=self.device, dtype=self.dtype)  # noqa: E731
        for li, L in enumerate(self.layers):
            p = f"model.layers.{li}."
            merged = {"qkv": ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "o": ("self_attn.o_proj",),
                      "gate_up": ("mlp.gate_proj", "mlp.up_proj"), "down": ("mlp.down_proj",)}
            for name, parts in merged.items():
                L[name].weight.copy_(torch.cat([t(p + part + ".weight") for part in parts], dim=0))
            for name, hf in (("in_norm", "input_layernorm"), ("post_attn_norm", "post_attention_layernorm"),
                             ("pre_ffn_norm", "pre_feedforward_layernorm"),
                             ("post_ffn_norm", "post_feedforward_layernorm")):
                L[name].copy_(t(p + hf + ".weight"))
        self.final_norm.copy_(t("model.norm.weight"))
        self.embed.copy_(t("model.embed_tokens.weight"))

    def reserve_workspaces(self, n_tokens: int, max_kv_len: int) -> None:
        """Grow the kernel workspaces once, before graph capture."""
        s = self.shape
        need = n_tokens * s.n_heads * 256 * (s.head_dim + 2) * 4   # worst-case split-KV partials
        need = max(need, 64 * n_tokens * max(2 * s.intermediate, s.hidden) * 4)
        widest = max(s.hidden, (s.n_heads + 2 * s.n_kv_heads) * s.head_dim)
        kernels.reserve_workspace(min(need, 4 << 30), self.device, deferred_nbytes=16 * n_tokens * widest * 4)

    def _trunk(self, tokens: torch.Tensor, positions: torch.Tensor, params: InputParameters) -> torch.Tensor:
        """Embedding and the decoder stack: the final-norm output of all T rows (a view of the static buffer)."""
        s, b = self.shape, self.buf
        T = tokens.numel()
        D, eps, defer = s.head_dim, s.rms_eps, self.defer_splitk
        nq, nkv = s.n_heads * D, s.n_kv_heads * D
        resid, normed, act = b["resid"][:T], b["normed"][:T], b["act"][:T]
        kernels.gemma_embed_norm(normed, resid, self.embed, tokens, self.embed_scale, self.layers[0]["in_norm"], eps)
        for li, L in enumerate(self.layers):
            qkv = L["qkv"].forward(normed, out=b["qkv"][:T], defer_splitk=defer)
            q = L["attn"].append(qkv[:, :nq], qkv[:, nq:nq + nkv], qkv[:, nq + nkv:], positions, L["kv"], params,
                                 qkv_partials=L["qkv"].deferred if defer else None)
            attn = L["attn"].decode(q, L["kv"], params, output=b["attn"][:T])
            o = L["o"].forward(attn, out=b["o"][:T], reduce=False, defer_splitk=defer)
            kernels.gemma_sandwich_norm(normed, o, L["post_attn_norm"], resid, L["pre_ffn_norm"], eps,
                                        partials=L["o"].deferred if defer else None)
            gu = L["gate_up"].forward(normed, out=b["gate_up"][:T])
            kernels.gelu_new_with_mul(gu, out=act)
            down = L["down"].forward(act, out=b["down"][:T], reduce=False, defer_splitk=defer)
            nxt = self.layers[li + 1]["in_norm"] if li + 1 < len(self.layers) else self.final_norm
            kernels.gemma_sandwich_norm(normed, down, L["post_ffn_norm"], resid, nxt, eps,
                                        partials=L["down"].deferred if defer else None)
        return normed

    def forward(self, tokens: torch.Tensor, positions: torch.Tensor, params: InputParameters,
                return_logits: bool = False, sampling=None):
        """tokens / positions [T] int32 -> next-token ids [n_seqs] (greedy) of each sequence's last token, or the
        soft-capped logits [n_seqs, vocab] (return_logits), or a sampling.SampleOutput over static buffers
        (sampling: sampling.SamplingParameters with >= n_seqs rows; the RNG position of a sequence is the position
        of its last input token)."""
        if sampling is not None and return_logits:
            raise ValueError("forward(): return_logits and sampling exclude each other")
        normed = self._trunk(tokens, positions, params)
        last = (params.q_cu_seq_lens[1:] - 1).long()
        self.last_hidden = normed[last]
        logits = self.last_hidden @ self.embed.t()   # plain library GEMM on the tied embedding, as the Llama step's
        kernels.soft_cap(logits, self.shape.final_logit_soft_cap)
        if sampling is not None:
            return self._sample(logits, positions[last], sampling)
        if return_logits:
            return logits
        return torch.argmax(logits, dim=-1).to(torch.int32)

    def _sample(self, logits: torch.Tensor, last_positions: torch.Tensor, sampling):
        """The fused sampling kernel over the capped logits into static output buffers (LlamaDecodeStep._sample)."""
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
