"""A torch-fp32 CPU restatement of the Qwen3 and Qwen3-MoE forwards (HuggingFace Qwen3ForCausalLM /
Qwen3MoeForCausalLM: Llama attention with an RMSNorm of every q and k head before RoPE, then a dense SiLU MLP or the
sparse mixture-of-experts block) with DENSE attention: the reference of tests/test_qwen3_step_gpu.py, pinned on the
installed HuggingFace models by tests/test_qwen3_ref_cpu.py.  Imports no GPU code.

It is tests/mixtral_model_ref.py's restatement (attention, routing, experts, and the `forced` selection explained
there) with the two per-head norms added; norm_topk_prob is the Mixtral model's `renormalize`.
"""
from dataclasses import dataclass, replace

import torch

from tests import mixtral_model_ref as M

rms_norm, rope, free_topk = M.rms_norm, M.rope, M.free_topk


@dataclass
class Qwen3RefConfig(M.MixtralRefConfig):
    n_experts: int = 0                 # 0: the dense MLP
    qk_norm: bool = True               # False: the control without q_norm / k_norm


class Qwen3Ref(M.MixtralRef):
    """layers: dicts of dense fp32 weights "qkv" [hidden, q | k | v], "o" [q, hidden] (x @ W), [head_dim] "q_norm",
    "k_norm", [hidden] "in_norm", "post_norm", and the MLP in the checkpoint's [out, in]: dense "w1" (gate), "w3" (up)
    [intermediate, hidden], "w2" (down) [hidden, intermediate], or per expert the same with a leading E and "gate"
    [E, hidden]; embed [vocab, hidden]; lm_head [hidden, vocab]."""

    def variant(self, **changes):
        return Qwen3Ref(self.layers, self.final_norm, self.embed, self.lm_head, replace(self.cfg, **changes))

    @torch.no_grad()
    def logits(self, tokens, forced=None, return_router=False):
        """[len(tokens), vocab] fp32 at every position of one sequence; forced / return_router as MixtralRef (MoE)"""
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
            q = qkv[:, :nq].reshape(T, c.n_heads, D)
            k = qkv[:, nq:nq + nkv].reshape(T, c.n_kv_heads, D)
            if c.qk_norm:
                q, k = rms_norm(q, W["q_norm"], c.rms_eps), rms_norm(k, W["k_norm"], c.rms_eps)
            q, k = rope(q, pos, c.rope_theta), rope(k, pos, c.rope_theta)
            v = qkv[:, nq + nkv:].reshape(T, c.n_kv_heads, D)
            h = h + self._attention(q, k, v) @ W["o"]
            x = rms_norm(h, W["post_norm"], c.rms_eps)
            if c.n_experts:
                y, r = self._moe(x, W, None if forced is None else forced[li])
                router.append(r)
            else:
                y = (torch.nn.functional.silu(x @ W["w1"].t()) * (x @ W["w3"].t())) @ W["w2"].t()
            h = h + y
        out = rms_norm(h, self.final_norm, c.rms_eps) @ self.lm_head
        return (out, router) if return_router else out


def from_hf(model) -> Qwen3Ref:
    """the restatement over the weights and configuration of a HuggingFace Qwen3ForCausalLM or Qwen3MoeForCausalLM
    (fp32): experts per expert (experts.{e}.gate_proj|up_proj|down_proj.weight) or fused into 3-D tensors
    experts.gate_up_proj [E, 2 I, H] (gate rows, then up rows) and experts.down_proj [E, H, I]"""
    cfg = model.config
    sd = {k: v.detach().float() for k, v in model.state_dict().items()}
    E = getattr(cfg, "num_experts", 0) or 0
    layers = []
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        t = lambda name: sd[p + name + ".weight"].t()  # noqa: E731
        W = {"qkv": torch.cat([t("self_attn.q_proj"), t("self_attn.k_proj"), t("self_attn.v_proj")], dim=1).contiguous(),
             "o": t("self_attn.o_proj").contiguous(), "q_norm": sd[p + "self_attn.q_norm.weight"],
             "k_norm": sd[p + "self_attn.k_norm.weight"], "in_norm": sd[p + "input_layernorm.weight"],
             "post_norm": sd[p + "post_attention_layernorm.weight"]}
        if E:
            W["gate"] = sd[p + "mlp.gate.weight"]
            if p + "mlp.experts.gate_up_proj" in sd:
                gu, w2 = sd[p + "mlp.experts.gate_up_proj"], sd[p + "mlp.experts.down_proj"]
                inter = gu.size(1) // 2
                w1, w3 = gu[:, :inter], gu[:, inter:]
            else:
                w1, w3, w2 = (torch.stack([sd[f"{p}mlp.experts.{e}.{w}.weight"] for e in range(E)])
                              for w in ("gate_proj", "up_proj", "down_proj"))
        else:
            w1, w3, w2 = (sd[f"{p}mlp.{w}.weight"] for w in ("gate_proj", "up_proj", "down_proj"))
        W.update(w1=w1.contiguous(), w3=w3.contiguous(), w2=w2.contiguous())
        layers.append(W)
    rope_theta = getattr(cfg, "rope_theta", None) or (getattr(cfg, "rope_parameters", None) or {}).get("rope_theta")
    lm_head = sd["model.embed_tokens.weight"] if cfg.tie_word_embeddings else sd["lm_head.weight"]
    return Qwen3Ref(layers, sd["model.norm.weight"], sd["model.embed_tokens.weight"], lm_head.t(), Qwen3RefConfig(
        n_heads=cfg.num_attention_heads, n_kv_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim,
        topk=getattr(cfg, "num_experts_per_tok", 0) if E else 0, rms_eps=cfg.rms_norm_eps,
        rope_theta=float(rope_theta), renormalize=bool(getattr(cfg, "norm_topk_prob", True)), n_experts=E))
