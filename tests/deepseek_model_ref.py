"""Torch CPU restatement of DeepSeek-V2's multi-head latent attention (HuggingFace DeepseekV2Attention), in the two
forms layers.MLAAttention rests on.  Imports no GPU code.

  naive     kv_b_proj expanded per token: k[t, h] = [W_UK[h] n[t] | rope(k_pe[t])], v[t, h] = W_UV[h] n[t];
            softmax(q k^T scale) v per head -- the HuggingFace forward.
  absorbed  q_lat[t, h] = q_nope[t, h] W_UK[h] (a vector of the latent width); attention over the latent rows n
            themselves, scores q_lat . n + q_pe . k_pe; out_lat W_UV[h]^T afterwards -- what the kernels run.

Both take the weights as a dict of [out, in] tensors under the checkpoint's names (q_proj | q_a_proj + q_a_layernorm
+ q_b_proj, kv_a_proj_with_mqa, kv_a_layernorm, kv_b_proj, o_proj) and run one whole sequence, causal, without a
cache: what a cached prefill / chunk / decode step gives at every position.  The dtype is the inputs' (float32 or
float64).  `rnd` in the absorbed form (default: identity) is applied wherever the kernel path stores a tensor in T,
so that absorbed(..., rnd=bf16 round trip) is the torch composition of the same arithmetic in bf16.
"""
from dataclasses import dataclass
from typing import Optional

import torch


@dataclass
class MLAConfig:
    n_heads: int
    nope: int
    rope: int
    v_dim: int
    latent: int
    q_lora_rank: Optional[int] = None
    eps: float = 1e-6
    sm_scale: Optional[float] = None      # None: (nope + rope) ** -0.5
    interleaved: bool = True              # HuggingFace's DeepSeek-V2 pairs (2i, 2i + 1)

    @property
    def scale(self):
        return self.sm_scale if self.sm_scale is not None else float(self.nope + self.rope) ** -0.5


def rms_norm(x, w, eps, rnd=lambda t: t):
    """T(T(x rs) w) under rnd, plain x rs w without"""
    return rnd(rnd(x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)) * w)


def rope(x, cos, sin, interleaved):
    """x [T, heads, D]; cos / sin [T, D / 2]"""
    c, s = cos[:, None, :], sin[:, None, :]
    if interleaved:
        a, b = x[..., 0::2], x[..., 1::2]
        return torch.stack([a * c - b * s, b * c + a * s], dim=-1).flatten(-2)
    half = x.size(-1) // 2
    a, b = x[..., :half], x[..., half:]
    return torch.cat([a * c - b * s, b * c + a * s], dim=-1)


def default_cos_sin(n_pos, rope_dim, theta=10000.0, dtype=torch.float32, inv_freq=None, attention_factor=1.0):
    """(cos, sin) [n_pos, rope / 2] in fp32 arithmetic (as the table the GPU is given), then cast"""
    if inv_freq is None:
        inv_freq = 1.0 / (theta ** (torch.arange(0, rope_dim, 2, dtype=torch.float32) / rope_dim))
    ang = torch.arange(n_pos, dtype=torch.float32)[:, None] * inv_freq.float()[None, :]
    return (ang.cos() * attention_factor).to(dtype), (ang.sin() * attention_factor).to(dtype)


def _project(x, W, cfg, cos, sin, rnd):
    """(q [T, H, nope + rope] with the tail rotated, n [T, latent], k_pe [T, rope] rotated)"""
    T, H, qk = x.size(0), cfg.n_heads, cfg.nope + cfg.rope
    if cfg.q_lora_rank is None:
        q = rnd(x @ W["q_proj"].t())
    else:
        q = rnd(rms_norm(rnd(x @ W["q_a_proj"].t()), W["q_a_layernorm"], cfg.eps, rnd) @ W["q_b_proj"].t())
    kv_a = rnd(x @ W["kv_a_proj_with_mqa"].t())
    q = q.view(T, H, qk)
    q = torch.cat([q[..., :cfg.nope], rnd(rope(q[..., cfg.nope:], cos, sin, cfg.interleaved))], dim=-1)
    n = rms_norm(kv_a[:, :cfg.latent], W["kv_a_layernorm"], cfg.eps, rnd)
    k_pe = rnd(rope(kv_a[:, None, cfg.latent:], cos, sin, cfg.interleaved))[:, 0]
    return q, n, k_pe


def _causal_softmax(s):
    T = s.size(-1)
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    return torch.softmax(s.masked_fill(~(j <= i)[None], float("-inf")), dim=-1)


def split_kv_b(W, cfg):
    """(W_UK [H, nope, latent], W_UV [H, v, latent]) from kv_b_proj [H (nope + v), latent]"""
    per_head = W["kv_b_proj"].view(cfg.n_heads, cfg.nope + cfg.v_dim, cfg.latent)
    return per_head[:, :cfg.nope], per_head[:, cfg.nope:]


@torch.no_grad()
def mla_naive(x, W, cfg, cos, sin, swap_uv=None):
    """x [T, hidden] -> o [T, hidden]: the HuggingFace form.  swap_uv = (h0, h1): the control of the GPU test, the
    value projections of two heads exchanged."""
    q, n, k_pe = _project(x, W, cfg, cos, sin, lambda t: t)
    w_uk, w_uv = split_kv_b(W, cfg)
    if swap_uv is not None:
        w_uv = w_uv.clone()
        w_uv[list(swap_uv)] = w_uv[list(reversed(swap_uv))]
    k_nope = torch.einsum("tl,hdl->thd", n, w_uk)
    v = torch.einsum("tl,hdl->thd", n, w_uv)
    k = torch.cat([k_nope, k_pe[:, None, :].expand(-1, cfg.n_heads, -1)], dim=-1)
    p = _causal_softmax(torch.einsum("ihd,jhd->hij", q, k) * cfg.scale)
    out = torch.einsum("hij,jhd->ihd", p, v).reshape(x.size(0), -1)
    return out @ W["o_proj"].t()


@torch.no_grad()
def mla_absorbed(x, W, cfg, cos, sin, rnd=lambda t: t):
    """the same function with the two halves of kv_b_proj absorbed into the query and the output"""
    q, n, k_pe = _project(x, W, cfg, cos, sin, rnd)
    w_uk, w_uv = split_kv_b(W, cfg)
    q_lat = rnd(torch.einsum("thd,hdl->thl", q[..., :cfg.nope], w_uk))
    s = (torch.einsum("ihl,jl->hij", q_lat, n) + torch.einsum("ihd,jd->hij", q[..., cfg.nope:], k_pe)) * cfg.scale
    out_lat = rnd(torch.einsum("hij,jl->ihl", _causal_softmax(s), n))
    v = rnd(torch.einsum("thl,hdl->thd", out_lat, w_uv))
    return rnd(v.reshape(x.size(0), -1) @ W["o_proj"].t())


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def random_mla_weights(cfg, hidden, seed, dtype=torch.float32, scale=None):
    """a seeded checkpoint under the HuggingFace names: [out, in] projections ~ N(0, 1 / in), norm weights near 1"""
    g = torch.Generator().manual_seed(seed)
    qk, H = cfg.nope + cfg.rope, cfg.n_heads
    lin = lambda n, k: (torch.randn(n, k, generator=g) * (scale or k ** -0.5)).to(dtype)  # noqa: E731
    W = {"kv_a_proj_with_mqa": lin(cfg.latent + cfg.rope, hidden),
         "kv_a_layernorm": (1 + 0.2 * torch.randn(cfg.latent, generator=g)).to(dtype),
         "kv_b_proj": lin(H * (cfg.nope + cfg.v_dim), cfg.latent), "o_proj": lin(hidden, H * cfg.v_dim)}
    if cfg.q_lora_rank is None:
        W["q_proj"] = lin(H * qk, hidden)
    else:
        W.update(q_a_proj=lin(cfg.q_lora_rank, hidden), q_b_proj=lin(H * qk, cfg.q_lora_rank),
                 q_a_layernorm=(1 + 0.2 * torch.randn(cfg.q_lora_rank, generator=g)).to(dtype))
    return W


# ---- the whole model ------------------------------------------------------------------------------------------------
@dataclass
class DeepseekRefConfig:
    mla: MLAConfig
    topk: int
    rms_eps: float = 1e-6
    norm_topk_prob: bool = False
    routed_scaling_factor: float = 1.0
    shared_experts: bool = True           # False: the control of the GPU test


def free_topk(r, k):
    """[T, E] router logits -> [T, k] int64: the k largest, equal values by ascending expert id"""
    import numpy as np
    return torch.from_numpy(np.argsort(-r.numpy(), axis=1, kind="stable")[:, :k].copy())


def _mlp(x, gate, up, down):
    return (torch.nn.functional.silu(x @ gate.t()) * (x @ up.t())) @ down.t()


class DeepseekV2Ref:
    """HuggingFace DeepseekV2ForCausalLM restated in torch fp32 with the NAIVE attention, one whole sequence at a
    time, no cache.  layers: dicts with "attn" (the dict mla_naive takes), "in_norm", "post_norm" and either the
    dense MLP "gate" | "up" | "down" ([out, in]) or the sparse one: "router" [E, hidden], "w1" | "w3" [E, I, hidden],
    "w2" [E, hidden, I] and the shared experts "shared_gate" | "shared_up" | "shared_down".  cos / sin [max_pos,
    rope / 2] hold whatever factor the RoPE variant multiplies in.

    Routing (topk_method greedy): weights = softmax over all experts at the k largest logits, divided by their sum
    under norm_topk_prob, times routed_scaling_factor.  `forced` replaces the SELECTION per sparse layer ([T, k]
    ids); the weights are still this model's own (tests/mixtral_model_ref.py explains why)."""

    def __init__(self, layers, final_norm, embed, lm_head, cos, sin, cfg: DeepseekRefConfig):
        self.layers, self.final_norm = layers, final_norm.float()
        self.embed, self.lm_head = embed.float(), lm_head.float()
        self.cos, self.sin, self.cfg = cos, sin, cfg

    def variant(self, layers=None, **changes):
        from dataclasses import replace
        return DeepseekV2Ref(layers or self.layers, self.final_norm, self.embed, self.lm_head, self.cos, self.sin,
                             replace(self.cfg, **changes))

    def _moe(self, x, W, sel):
        c = self.cfg
        r = x @ W["router"].t()
        if sel is None:
            sel = free_topk(r, c.topk)
        import numpy as np
        sel = torch.as_tensor(np.asarray(sel), dtype=torch.long)
        w = torch.softmax(r, dim=-1).gather(1, sel)
        if c.norm_topk_prob:
            w = w / w.sum(-1, keepdim=True)
        w = w * c.routed_scaling_factor
        out = torch.zeros_like(x)
        for e in sel.unique().tolist():
            t, j = (sel == e).nonzero(as_tuple=True)
            out.index_add_(0, t, _mlp(x[t], W["w1"][e], W["w3"][e], W["w2"][e]) * w[t, j][:, None])
        if c.shared_experts:
            out = out + _mlp(x, W["shared_gate"], W["shared_up"], W["shared_down"])
        return out, r

    @torch.no_grad()
    def logits(self, tokens, forced=None, return_router=False):
        """[len(tokens), vocab] fp32.  forced: per SPARSE layer the [T, k] expert ids (None: free);
        return_router: also the router logits [T, E] of every sparse layer"""
        c = self.cfg
        tokens = torch.as_tensor(tokens, dtype=torch.long)
        T = tokens.numel()
        cos, sin = self.cos[:T], self.sin[:T]
        h = self.embed[tokens]
        router, si = [], 0
        for W in self.layers:
            x = rms_norm(h, W["in_norm"], c.rms_eps)
            h = h + mla_naive(x, W["attn"], c.mla, cos, sin)
            x = rms_norm(h, W["post_norm"], c.rms_eps)
            if "router" in W:
                y, r = self._moe(x, W, None if forced is None else forced[si])
                router.append(r)
                si += 1
            else:
                y = _mlp(x, W["gate"], W["up"], W["down"])
            h = h + y
        out = rms_norm(h, self.final_norm, c.rms_eps) @ self.lm_head
        return (out, router) if return_router else out


def from_hf(model) -> DeepseekV2Ref:
    """the restatement over the weights and configuration of a HuggingFace DeepseekV2ForCausalLM (fp32).  The RoPE
    frequencies and the factor on cos | sin are read from the model's rotary module, the softmax scale from its
    attention (both are checked against scalellm_amd.deepseek's host formulas by tests/test_deepseek_ref_cpu.py)."""
    cfg = model.config
    sd = {k: v.detach().float() for k, v in model.state_dict().items()}
    mla = MLAConfig(n_heads=cfg.num_attention_heads, nope=cfg.qk_nope_head_dim, rope=cfg.qk_rope_head_dim,
                    v_dim=cfg.v_head_dim, latent=cfg.kv_lora_rank, q_lora_rank=cfg.q_lora_rank, eps=cfg.rms_norm_eps,
                    sm_scale=float(model.model.layers[0].self_attn.scaling), interleaved=True)
    layers = []
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        names = ["kv_a_proj_with_mqa", "kv_a_layernorm", "kv_b_proj", "o_proj"] + \
            (["q_proj"] if cfg.q_lora_rank is None else ["q_a_proj", "q_a_layernorm", "q_b_proj"])
        W = {"attn": {n: sd[f"{p}self_attn.{n}.weight"] for n in names},
             "in_norm": sd[p + "input_layernorm.weight"], "post_norm": sd[p + "post_attention_layernorm.weight"]}
        if p + "mlp.gate.weight" in sd:
            gu, w2 = sd[p + "mlp.experts.gate_up_proj"], sd[p + "mlp.experts.down_proj"]
            inter = gu.size(1) // 2
            W.update(router=sd[p + "mlp.gate.weight"], w1=gu[:, :inter].contiguous(), w3=gu[:, inter:].contiguous(),
                     w2=w2.contiguous(), shared_gate=sd[p + "mlp.shared_experts.gate_proj.weight"],
                     shared_up=sd[p + "mlp.shared_experts.up_proj.weight"],
                     shared_down=sd[p + "mlp.shared_experts.down_proj.weight"])
        else:
            W.update(gate=sd[p + "mlp.gate_proj.weight"], up=sd[p + "mlp.up_proj.weight"],
                     down=sd[p + "mlp.down_proj.weight"])
        layers.append(W)
    rot = model.model.rotary_emb
    cos, sin = default_cos_sin(cfg.max_position_embeddings, cfg.qk_rope_head_dim, inv_freq=rot.inv_freq.float(),
                               attention_factor=float(rot.attention_scaling))
    return DeepseekV2Ref(layers, sd["model.norm.weight"], sd["model.embed_tokens.weight"], sd["lm_head.weight"].t(),
                         cos, sin, DeepseekRefConfig(mla=mla, topk=cfg.num_experts_per_tok, rms_eps=cfg.rms_norm_eps,
                                                     norm_topk_prob=False,
                                                     routed_scaling_factor=float(cfg.routed_scaling_factor)))
