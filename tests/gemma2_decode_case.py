"""The case of tests/test_gemma2_decode_step_gpu.py and its references, on the CPU (imports no GPU code): a tiny
random Gemma-2 checkpoint in HuggingFace's names, two sequences with 20 cached tokens and three decode steps, and a
plain PyTorch Gemma-2 forward that runs in fp32 (THE reference) or in bf16 as a framework would (HuggingFace's eager
path: bf16 matmuls, RMSNorm and softmax computed in fp32 and cast back), which is where the tolerance comes from.

2 layers -- layer 0 with the sliding window, layer 1 without --, hidden 256, 2 query heads on 1 KV head of 256,
intermediate 512, vocab 512, window 16 (HuggingFace's count: the query's own key included), caps 50 / 30,
query_pre_attn_scalar 144 (not head_dim).  Every tensor is drawn in fp32 and rounded to bf16 once: both references
and the step under test start from the same bf16 values.

TOLERANCES, measured here on this seed (tests/test_gemma2_decode_ref_cpu.py re-measures and brackets them): the bf16
run against the fp32 reference over the three steps,
    logits      relative L2 error  9.18e-3  (BF16_LOGITS_ERR)
    appended K  relative L2 error  5.72e-3  (BF16_K_ERR; both layers, after RoPE)
    appended V  relative L2 error  5.09e-3  (BF16_V_ERR)
and the bound of the GPU test is twice each (1.836e-2, 1.144e-2, 1.018e-2): the fused path should be no worse than a
bf16 framework path, and the factor leaves room for another order of accumulation."""
import torch
import torch.nn.functional as F

HF_CONFIG = dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, head_dim=256, intermediate_size=512,
                 num_hidden_layers=2, vocab_size=512, sliding_window=16, query_pre_attn_scalar=144,
                 attn_logit_softcapping=50.0, final_logit_softcapping=30.0, rope_theta=10000.0, rms_norm_eps=1e-6,
                 max_position_embeddings=128)
N_SEQS, PREFILL, N_DECODE, SEED = 2, 20, 3, 20
BF16_LOGITS_ERR, BF16_K_ERR, BF16_V_ERR = 9.18e-3, 5.72e-3, 5.09e-3
TOL_LOGITS, TOL_K, TOL_V = 2 * BF16_LOGITS_ERR, 2 * BF16_K_ERR, 2 * BF16_V_ERR

_LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj",
            "mlp.up_proj", "mlp.down_proj")
_NORMS = ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm")


def checkpoint():
    """HuggingFace-named bf16 tensors.  Linear weights [out, in] with variance 1 / in (unit-variance activations
    stay so, and the attention scores reach the curved part of the soft cap), norm weights the checkpoint's w of
    (1 + w), a tied embedding."""
    c = HF_CONFIG
    g = torch.Generator().manual_seed(SEED)
    nq, nkv, hid, inter = c["num_attention_heads"] * c["head_dim"], c["num_key_value_heads"] * c["head_dim"], \
        c["hidden_size"], c["intermediate_size"]
    shapes = {"self_attn.q_proj": (nq, hid), "self_attn.k_proj": (nkv, hid), "self_attn.v_proj": (nkv, hid),
              "self_attn.o_proj": (hid, nq), "mlp.gate_proj": (inter, hid), "mlp.up_proj": (inter, hid),
              "mlp.down_proj": (hid, inter)}
    sd = {}
    for i in range(c["num_hidden_layers"]):
        for name in _LINEARS:
            n, k = shapes[name]
            sd[f"model.layers.{i}.{name}.weight"] = (torch.randn(n, k, generator=g) * k ** -0.5).bfloat16()
        for name in _NORMS:
            sd[f"model.layers.{i}.{name}.weight"] = (0.3 * torch.randn(hid, generator=g)).bfloat16()
    sd["model.norm.weight"] = (0.3 * torch.randn(hid, generator=g)).bfloat16()
    sd["model.embed_tokens.weight"] = (torch.randn(c["vocab_size"], hid, generator=g) * hid ** -0.5).bfloat16()
    return sd


def tokens():
    """[N_SEQS, PREFILL + N_DECODE] int64: the decode steps are teacher-forced, so every side sees the same inputs"""
    g = torch.Generator().manual_seed(SEED + 1)
    return torch.randint(0, HF_CONFIG["vocab_size"], (N_SEQS, PREFILL + N_DECODE), generator=g)


def _norm(x, w, eps, dtype):
    """Gemma2RMSNorm: fp32 inside, (1 + w), cast back"""
    x = x.float()
    return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * (1.0 + w.float())).to(dtype)


def _rope(x, theta):
    """[T, heads, D] at positions 0 .. T - 1, pairs (i, i + D / 2) (neox), the table in fp32"""
    T, _, D = x.shape
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
    c, s = ang.cos()[:, None, :].to(x.dtype), ang.sin()[:, None, :].to(x.dtype)
    a, b = x[..., :D // 2], x[..., D // 2:]
    return torch.cat([a * c - b * s, b * c + a * s], dim=-1)


@torch.no_grad()
def forward(sd, toks, dtype=torch.float32, window=None, attn_cap=None):
    """One sequence, all positions at once (what a cache and decode steps give position by position).  Returns
    (logits [T, vocab], [(k [T, kv_heads, D] after RoPE, v [T, kv_heads, D]) per layer]), in dtype.
    window / attn_cap override the configuration's (the controls of the tests); window 0 = off."""
    c = HF_CONFIG
    window = c["sliding_window"] if window is None else window
    cap = c["attn_logit_softcapping"] if attn_cap is None else attn_cap
    H, HKV, D, eps = c["num_attention_heads"], c["num_key_value_heads"], c["head_dim"], c["rms_norm_eps"]
    W = lambda name: sd[name].to(dtype)  # noqa: E731
    T = toks.numel()
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    h = W("model.embed_tokens.weight")[toks] * torch.tensor(c["hidden_size"] ** 0.5, dtype=dtype)
    kv = []
    for li in range(c["num_hidden_layers"]):
        p = f"model.layers.{li}."
        x = _norm(h, sd[p + "input_layernorm.weight"], eps, dtype)
        q = _rope((x @ W(p + "self_attn.q_proj.weight").t()).view(T, H, D), c["rope_theta"])
        k = _rope((x @ W(p + "self_attn.k_proj.weight").t()).view(T, HKV, D), c["rope_theta"])
        v = (x @ W(p + "self_attn.v_proj.weight").t()).view(T, HKV, D)
        kv.append((k, v))
        kr, vr = k.repeat_interleave(H // HKV, dim=1), v.repeat_interleave(H // HKV, dim=1)
        s = torch.einsum("ihd,jhd->hij", q, kr) * c["query_pre_attn_scalar"] ** -0.5
        if cap > 0:
            s = torch.tanh(s / cap) * cap
        visible = j <= i
        if li % 2 == 0 and window > 0:       # the query at i sees the keys j > i - window
            visible = visible & (j > i - window)
        s = s.masked_fill(~visible[None], float("-inf"))
        a = torch.einsum("hij,jhd->ihd", torch.softmax(s, dim=-1, dtype=torch.float32).to(dtype), vr).reshape(T, H * D)
        h = _norm(a @ W(p + "self_attn.o_proj.weight").t(), sd[p + "post_attention_layernorm.weight"], eps, dtype) + h
        x = _norm(h, sd[p + "pre_feedforward_layernorm.weight"], eps, dtype)
        act = F.gelu(x @ W(p + "mlp.gate_proj.weight").t(), approximate="tanh") * (x @ W(p + "mlp.up_proj.weight").t())
        h = _norm(act @ W(p + "mlp.down_proj.weight").t(), sd[p + "post_feedforward_layernorm.weight"], eps, dtype) + h
    logits = _norm(h, sd["model.norm.weight"], eps, dtype) @ W("model.embed_tokens.weight").t()
    fc = c["final_logit_softcapping"]
    return torch.tanh(logits / fc) * fc, kv


def decode_rows(sd, toks, **kw):
    """what the three decode steps produce, over both sequences: logits [N_DECODE, N_SEQS, vocab] and per layer
    K, V [N_DECODE, N_SEQS, kv_heads, D] of the appended rows, all as fp32; and per layer the K, V of the PREFILL
    tokens [N_SEQS, PREFILL, kv_heads, D] (what the cache holds before the first step)"""
    runs = [forward(sd, toks[s], **kw) for s in range(N_SEQS)]
    logits = torch.stack([r[0][PREFILL:].float() for r in runs], dim=1)
    n_layers = HF_CONFIG["num_hidden_layers"]
    new = [tuple(torch.stack([r[1][li][x][PREFILL:].float() for r in runs], dim=1) for x in (0, 1))
           for li in range(n_layers)]
    old = [tuple(torch.stack([r[1][li][x][:PREFILL] for r in runs]) for x in (0, 1)) for li in range(n_layers)]
    return logits, new, old


def rel_l2(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())
