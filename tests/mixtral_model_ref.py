"""A torch-fp32 CPU restatement of the Mixtral forward (HuggingFace MixtralForCausalLM: Llama attention block, sparse
mixture-of-experts FFN) with DENSE attention: the reference of tests/test_mixtral_step_gpu.py, pinned on the
installed MixtralForCausalLM by tests/test_moe_router_cpu.py.  Imports no GPU code.

The model keeps no cache: logits(tokens) runs the whole sequence, which gives at every position what a cached
prefill / chunk / decode step gives there.

Routing.  r = x . gate^T; the k experts with the largest r (ties: the lower id); weights = softmax over ALL experts
at those, divided by their sum when cfg.renormalize (Mixtral's rule).  `forced` replaces the SELECTION per layer
([T, k] expert ids): the weights are still computed from this model's own logits at those experts.  With it a
comparison against an implementation in lower precision can use that implementation's own selections, so that no
token has to be left out because a near-tie fell the other way.
"""
from dataclasses import dataclass, replace

import numpy as np
import torch


@dataclass
class MixtralRefConfig:
    n_heads: int
    n_kv_heads: int
    head_dim: int
    topk: int
    rms_eps: float = 1e-5
    rope_theta: float = 1e6
    renormalize: bool = True


def rms_norm(x, w, eps):
    x = x.float()
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w.float()


def rope(x, positions, theta):
    """[T, heads, D], non-interleaved pairs (i, i + D / 2)"""
    D = x.size(-1)
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = positions.float()[:, None] * inv[None, :]
    c, s = ang.cos()[:, None, :], ang.sin()[:, None, :]
    a, b = x[..., :D // 2], x[..., D // 2:]
    return torch.cat([a * c - b * s, b * c + a * s], dim=-1)


def free_topk(r, k):
    """[T, E] router logits -> [T, k] int64: the k largest, equal values by ascending expert id"""
    return torch.from_numpy(np.argsort(-r.numpy(), axis=1, kind="stable")[:, :k].copy())


class MixtralRef:
    """layers: dicts of dense fp32 weights "qkv" [hidden, q | k | v], "o" [q, hidden] (x @ W), "gate" [E, hidden],
    "w1", "w3" [E, intermediate, hidden], "w2" [E, hidden, intermediate] (the checkpoint's [out, in]) and [hidden]
    norm weights "in_norm", "post_norm"; embed [vocab, hidden]; lm_head [hidden, vocab]."""

    def __init__(self, layers, final_norm, embed, lm_head, cfg: MixtralRefConfig):
        self.layers, self.final_norm, self.embed, self.lm_head = layers, final_norm.float(), embed.float(), lm_head.float()
        self.cfg = cfg

    def variant(self, **changes):
        """the same weights under a changed configuration (the controls of the GPU test)"""
        return MixtralRef(self.layers, self.final_norm, self.embed, self.lm_head, replace(self.cfg, **changes))

    def _attention(self, q, k, v):
        c = self.cfg
        T = q.size(0)
        group = c.n_heads // c.n_kv_heads
        k, v = k.repeat_interleave(group, dim=1), v.repeat_interleave(group, dim=1)
        s = torch.einsum("ihd,jhd->hij", q, k) * float(c.head_dim) ** -0.5
        i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
        s = s.masked_fill(~(j <= i)[None], float("-inf"))
        return torch.einsum("hij,jhd->ihd", torch.softmax(s, dim=-1), v).reshape(T, -1)

    def _moe(self, x, W, sel):
        """x [T, hidden] -> (out [T, hidden], router logits [T, E]); sel: forced [T, k] ids or None"""
        c = self.cfg
        r = x @ W["gate"].t()
        if sel is None:
            sel = free_topk(r, c.topk)
        sel = torch.as_tensor(np.asarray(sel), dtype=torch.long)
        w = torch.softmax(r, dim=-1).gather(1, sel)
        if c.renormalize:
            w = w / w.sum(-1, keepdim=True)
        out = torch.zeros_like(x)
        for e in sel.unique().tolist():
            t, j = (sel == e).nonzero(as_tuple=True)
            xe = x[t]
            y = (torch.nn.functional.silu(xe @ W["w1"][e].t()) * (xe @ W["w3"][e].t())) @ W["w2"][e].t()
            out.index_add_(0, t, y * w[t, j][:, None])
        return out, r

    @torch.no_grad()
    def logits(self, tokens, forced=None, return_router=False):
        """[len(tokens), vocab] fp32: the logits at every position of one sequence.  forced: per layer, the [T, k]
        expert ids to use in place of this model's own top-k (None: free).  return_router: also the per-layer
        router logits [T, E]."""
        c = self.cfg
        tokens = torch.as_tensor(tokens, dtype=torch.long)
        T, D = tokens.numel(), c.head_dim
        pos = torch.arange(T)
        nq, nkv = c.n_heads * D, c.n_kv_heads * D
        h = self.embed[tokens]
        router = []
        for li, W in enumerate(self.layers):
            x = rms_norm(h, W["in_norm"], c.rms_eps)
            qkv = x @ W["qkv"]
            q = rope(qkv[:, :nq].reshape(T, c.n_heads, D), pos, c.rope_theta)
            k = rope(qkv[:, nq:nq + nkv].reshape(T, c.n_kv_heads, D), pos, c.rope_theta)
            v = qkv[:, nq + nkv:].reshape(T, c.n_kv_heads, D)
            h = h + self._attention(q, k, v) @ W["o"]
            x = rms_norm(h, W["post_norm"], c.rms_eps)
            y, r = self._moe(x, W, None if forced is None else forced[li])
            router.append(r)
            h = h + y
        out = rms_norm(h, self.final_norm, c.rms_eps) @ self.lm_head
        return (out, router) if return_router else out


def from_hf(model) -> MixtralRef:
    """the restatement over the weights and configuration of a HuggingFace MixtralForCausalLM (fp32), whichever
    parameter names the installed version uses: per-expert experts.{e}.w1|w2|w3.weight, or the experts fused into
    3-D tensors experts.gate_up_proj [E, 2 I, H] (gate rows, then up rows) and experts.down_proj [E, H, I]."""
    cfg = model.config
    sd = {k: v.detach().float() for k, v in model.state_dict().items()}
    E = cfg.num_local_experts
    layers = []
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        t = lambda name: sd[p + name + ".weight"].t()  # noqa: E731
        moe = next(m for m in ("block_sparse_moe.", "mlp.") if p + m + "gate.weight" in sd)
        if p + moe + "experts.gate_up_proj" in sd:
            gu, w2 = sd[p + moe + "experts.gate_up_proj"], sd[p + moe + "experts.down_proj"]
            inter = gu.size(1) // 2
            w1, w3 = gu[:, :inter], gu[:, inter:]
        else:
            w1, w3, w2 = (torch.stack([sd[f"{p}{moe}experts.{e}.{w}.weight"] for e in range(E)])
                          for w in ("w1", "w3", "w2"))
        layers.append({
            "qkv": torch.cat([t("self_attn.q_proj"), t("self_attn.k_proj"), t("self_attn.v_proj")], dim=1).contiguous(),
            "o": t("self_attn.o_proj").contiguous(), "gate": sd[p + moe + "gate.weight"],
            "w1": w1.contiguous(), "w3": w3.contiguous(), "w2": w2.contiguous(),
            "in_norm": sd[p + "input_layernorm.weight"], "post_norm": sd[p + "post_attention_layernorm.weight"]})
    rope_theta = getattr(cfg, "rope_theta", None) or (getattr(cfg, "rope_parameters", None) or {}).get("rope_theta", 1e6)
    head_dim = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
    return MixtralRef(layers, sd["model.norm.weight"], sd["model.embed_tokens.weight"], sd["lm_head.weight"].t(),
                      MixtralRefConfig(n_heads=cfg.num_attention_heads, n_kv_heads=cfg.num_key_value_heads,
                                       head_dim=head_dim, topk=cfg.num_experts_per_tok, rms_eps=cfg.rms_norm_eps,
                                       rope_theta=float(rope_theta)))
