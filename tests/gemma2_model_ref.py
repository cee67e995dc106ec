"""A torch-fp32 CPU restatement of the reference's Gemma-2 forward (src/models/google/gemma2.h:128-139, 186-204,
263-276, 333-343) with DENSE attention: the reference of tests/test_gemma2_step_gpu.py, pinned on HuggingFace
Gemma2ForCausalLM by tests/test_gemma2_ref_cpu.py.  Imports no GPU code.

The mask is the reference's: with the query at position i of its sequence, key j is visible when 0 <= i - j <= W
(attention handler: tril(diag) & triu(diag - W)), so a window W keeps W + 1 keys; W < 0 is no window.  The window
applies on EVEN layers (gemma2.h:249-251).  The model keeps no cache: logits(tokens) runs the whole sequence, which
gives at every position what a cached prefill / chunk / decode step gives there.
"""
from dataclasses import dataclass, replace

import torch


@dataclass
class Gemma2RefConfig:
    n_heads: int
    n_kv_heads: int
    head_dim: int
    rms_eps: float = 1e-6
    rope_theta: float = 10000.0
    attn_scalar: float = 256.0
    sliding_window: int = 4096          # the reference's W; < 0: off
    attn_logit_soft_cap: float = 50.0
    final_logit_soft_cap: float = 30.0
    embed_scale: float = 0.0            # 0: sqrt(hidden) in fp32; the reference uses T(sqrt(hidden)) (gemma2.h:236-238)
    sm_scale: float = 0.0               # 0: attn_scalar ** -0.5


def gemma_rms_norm(x, w, eps):
    """detail::gemma_rms_norm (src/layers/normalization.h:31-40) in fp32"""
    x = x.float()
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * (1.0 + w.float())


def rope(x, positions, theta):
    """[T, heads, D], non-interleaved pairs (i, i + D / 2)"""
    D = x.size(-1)
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = positions.float()[:, None] * inv[None, :]
    c, s = ang.cos()[:, None, :], ang.sin()[:, None, :]
    a, b = x[..., :D // 2], x[..., D // 2:]
    return torch.cat([a * c - b * s, b * c + a * s], dim=-1)


class Gemma2Ref:
    """layers: dicts of dense fp32 [K, N] weights "qkv" (q | k | v columns), "o", "gate_up" (gate | up), "down" and
    [hidden] norm weights "in_norm", "post_attn_norm", "pre_ffn_norm", "post_ffn_norm"; embed [vocab, hidden] is
    the lm_head as well (gemma2.h:311)."""

    def __init__(self, layers, final_norm, embed, cfg: Gemma2RefConfig):
        self.layers, self.final_norm, self.embed, self.cfg = layers, final_norm.float(), embed.float(), cfg

    def variant(self, **changes):
        """the same weights under a changed configuration (the controls of the GPU test)"""
        return Gemma2Ref(self.layers, self.final_norm, self.embed, replace(self.cfg, **changes))

    def _attention(self, q, k, v, li):
        c = self.cfg
        T = q.size(0)
        group = c.n_heads // c.n_kv_heads
        k, v = k.repeat_interleave(group, dim=1), v.repeat_interleave(group, dim=1)
        scale = c.sm_scale if c.sm_scale else float(c.attn_scalar) ** -0.5
        s = torch.einsum("ihd,jhd->hij", q, k) * scale
        if c.attn_logit_soft_cap > 0:
            s = torch.tanh(s / c.attn_logit_soft_cap) * c.attn_logit_soft_cap
        i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
        visible = j <= i
        if li % 2 == 0 and c.sliding_window >= 0:
            visible = visible & (i - j <= c.sliding_window)
        s = s.masked_fill(~visible[None], float("-inf"))
        return torch.einsum("hij,jhd->ihd", torch.softmax(s, dim=-1), v).reshape(T, -1)

    @torch.no_grad()
    def logits(self, tokens):
        """[len(tokens), vocab] fp32: the capped logits at every position of one sequence"""
        c = self.cfg
        tokens = torch.as_tensor(tokens, dtype=torch.long)
        T, D = tokens.numel(), c.head_dim
        pos = torch.arange(T)
        nq, nkv = c.n_heads * D, c.n_kv_heads * D
        h = self.embed[tokens] * (c.embed_scale if c.embed_scale else float(self.embed.size(1)) ** 0.5)
        for li, W in enumerate(self.layers):
            x = gemma_rms_norm(h, W["in_norm"], c.rms_eps)
            qkv = x @ W["qkv"]
            q = rope(qkv[:, :nq].reshape(T, c.n_heads, D), pos, c.rope_theta)
            k = rope(qkv[:, nq:nq + nkv].reshape(T, c.n_kv_heads, D), pos, c.rope_theta)
            v = qkv[:, nq + nkv:].reshape(T, c.n_kv_heads, D)
            a = self._attention(q, k, v, li) @ W["o"]
            h = gemma_rms_norm(a, W["post_attn_norm"], c.rms_eps) + h
            x = gemma_rms_norm(h, W["pre_ffn_norm"], c.rms_eps)
            gu = x @ W["gate_up"]
            inter = gu.size(1) // 2
            act = torch.nn.functional.gelu(gu[:, :inter], approximate="tanh") * gu[:, inter:]
            h = gemma_rms_norm(act @ W["down"], W["post_ffn_norm"], c.rms_eps) + h
        out = gemma_rms_norm(h, self.final_norm, c.rms_eps) @ self.embed.t()
        return torch.tanh(out / c.final_logit_soft_cap) * c.final_logit_soft_cap


def from_hf(model) -> Gemma2Ref:
    """the restatement over the weights and configuration of a HuggingFace Gemma2ForCausalLM (fp32).  HF's
    sliding_window counts the keys a query sees, itself included; the reference's W counts the keys BEHIND it:
    W = sliding_window - 1 (asserted, with its neighbours, by tests/test_gemma2_ref_cpu.py)."""
    cfg = model.config
    sd = {k: v.detach().float() for k, v in model.state_dict().items()}
    layers = []
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        t = lambda name: sd[p + name + ".weight"].t()  # noqa: E731
        layers.append({
            "qkv": torch.cat([t("self_attn.q_proj"), t("self_attn.k_proj"), t("self_attn.v_proj")], dim=1).contiguous(),
            "o": t("self_attn.o_proj").contiguous(),
            "gate_up": torch.cat([t("mlp.gate_proj"), t("mlp.up_proj")], dim=1).contiguous(),
            "down": t("mlp.down_proj").contiguous(),
            "in_norm": sd[p + "input_layernorm.weight"], "post_attn_norm": sd[p + "post_attention_layernorm.weight"],
            "pre_ffn_norm": sd[p + "pre_feedforward_layernorm.weight"],
            "post_ffn_norm": sd[p + "post_feedforward_layernorm.weight"]})
    rope_theta = getattr(cfg, "rope_theta", None) or (getattr(cfg, "rope_parameters", None) or {}).get("rope_theta", 10000.0)
    return Gemma2Ref(layers, sd["model.norm.weight"], sd["model.embed_tokens.weight"], Gemma2RefConfig(
        n_heads=cfg.num_attention_heads, n_kv_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim,
        rms_eps=cfg.rms_norm_eps, rope_theta=float(rope_theta), attn_scalar=float(cfg.query_pre_attn_scalar),
        sliding_window=cfg.sliding_window - 1, attn_logit_soft_cap=float(cfg.attn_logit_softcapping),
        final_logit_soft_cap=float(cfg.final_logit_softcapping)))
