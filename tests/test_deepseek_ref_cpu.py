"""The DeepSeek-V2 reference of tests/deepseek_model_ref.py, without a GPU:
  * pinned on the installed transformers.DeepseekV2ForCausalLM with seeded random weights at the tiny and tiny_qlora
    configurations, default and yarn RoPE, at the bound tests/test_moe_router_cpu.py uses for the Mixtral pin,
  * the absorbed form (q W_UK, attention over the latent, then W_UV) equals the naive one in float64: the identity
    layers.MLAAttention rests on,
  * the host-built YaRN table and softmax scale of scalellm_amd/deepseek.py equal transformers' yarn init,
  * what DeepseekV2DecodeStep refuses is refused before a GPU is touched.
"""
import numpy as np
import pytest
import torch

from scalellm_amd import deepseek
from tests import deepseek_model_ref as R
from tests.e2e_common import check_logits, rel_l2

TOL = 1e-4                           # the Mixtral, Llama and Gemma-2 pins' bound: torch's fp32 noise
SEQ_LEN = 24
YARN = dict(rope_type="yarn", rope_factor=8.0, original_max_position=64, mscale=0.707, mscale_all_dim=1.0)


def _shape(qlora, yarn):
    s = deepseek.DeepseekV2Shape.tiny_qlora() if qlora else deepseek.DeepseekV2Shape.tiny()
    for k, v in (YARN if yarn else {}).items():
        setattr(s, k, v)
    return s


def _hf_model(s):
    transformers = pytest.importorskip("transformers")
    mm = pytest.importorskip("transformers.models.deepseek_v2.modeling_deepseek_v2")
    rope = dict(rope_type="default", rope_theta=s.rope_theta)
    if s.rope_type == "yarn":
        rope = dict(rope_type="yarn", rope_theta=s.rope_theta, factor=s.rope_factor,
                    original_max_position_embeddings=s.original_max_position, beta_fast=s.beta_fast,
                    beta_slow=s.beta_slow, mscale=s.mscale, mscale_all_dim=s.mscale_all_dim)
    cfg = transformers.DeepseekV2Config(
        hidden_size=s.hidden, num_attention_heads=s.n_heads, num_key_value_heads=s.n_heads,
        qk_nope_head_dim=s.nope_head_dim, qk_rope_head_dim=s.rope_head_dim, v_head_dim=s.v_head_dim,
        kv_lora_rank=s.kv_lora_rank, q_lora_rank=s.q_lora_rank, intermediate_size=s.intermediate,
        moe_intermediate_size=s.moe_intermediate, n_routed_experts=s.n_routed_experts,
        n_shared_experts=s.n_shared_experts, num_experts_per_tok=s.topk, first_k_dense_replace=s.first_k_dense_replace,
        num_hidden_layers=s.n_layers, vocab_size=s.vocab, max_position_embeddings=s.max_position,
        rms_norm_eps=s.rms_eps, topk_method="greedy", routed_scaling_factor=1.0, norm_topk_prob=False,
        attention_bias=False, attention_dropout=0.0, tie_word_embeddings=False, rope_parameters=rope)
    cfg._attn_implementation = "eager"
    torch.manual_seed(7)
    model = mm.DeepseekV2ForCausalLM(cfg).eval().float()
    with torch.no_grad():                                          # make every term matter
        for name, p in model.named_parameters():
            if name.endswith("norm.weight") or "layernorm" in name:
                p.copy_(1 + 0.3 * torch.randn_like(p))
            elif "mlp.gate.weight" in name:
                p.copy_(0.5 * torch.randn_like(p))
            else:
                p.copy_(0.1 * torch.randn_like(p))
    return model


@pytest.fixture(scope="module", params=[(False, False), (True, False), (False, True), (True, True)],
                ids=["tiny", "tiny_qlora", "tiny-yarn", "tiny_qlora-yarn"])
def pinned(request):
    s = _shape(*request.param)
    model = _hf_model(s)
    tokens = torch.from_numpy(np.random.default_rng(11).integers(0, s.vocab, size=SEQ_LEN))
    with torch.no_grad():
        ref = model(input_ids=tokens[None]).logits[0].float().numpy()
    return s, model, ref, tokens


def test_restatement_matches_hf_deepseek_v2(pinned):
    s, model, ref, tokens = pinned
    ours = R.from_hf(model)
    n_sparse = s.n_layers - s.first_k_dense_replace
    got, router = ours.logits(tokens, return_router=True)
    same, n, rel = check_logits(got.numpy(), ref, TOL, "restatement vs HF DeepseekV2ForCausalLM")
    print(f"\n[deepseek-ref] {s.rope_type} q_lora {s.q_lora_rank}: rel L2 {rel:.2e}, greedy ids equal in {same} of {n}")
    assert len(router) == n_sparse and router[0].shape == (SEQ_LEN, s.n_routed_experts)
    own = [R.free_topk(r, s.topk) for r in router]
    assert torch.equal(ours.logits(tokens, forced=own), got)       # forcing the model's own selection changes nothing
    # every DeepSeek term is held in place by the pin: each change moves the logits past the bound
    E = s.n_routed_experts
    assert rel_l2(ours.variant(shared_experts=False).logits(tokens).numpy(), ref) > 10 * TOL
    assert rel_l2(ours.variant(norm_topk_prob=True).logits(tokens).numpy(), ref) > 10 * TOL
    assert rel_l2(ours.logits(tokens, forced=[(o + 1) % E for o in own]).numpy(), ref) > 10 * TOL
    ones = [dict(W, attn=dict(W["attn"], kv_a_layernorm=torch.ones_like(W["attn"]["kv_a_layernorm"])))
            for W in ours.layers]
    assert rel_l2(ours.variant(layers=ones).logits(tokens).numpy(), ref) > 10 * TOL
    other = R.MLAConfig(**{**ours.cfg.mla.__dict__, "interleaved": False})
    assert rel_l2(ours.variant(mla=other).logits(tokens).numpy(), ref) > 10 * TOL


def test_host_rope_table_and_scale_are_the_models(pinned):
    """scalellm_amd.deepseek's table (default, or yarn: blended frequencies, the attention factor on cos | sin) and
    softmax scale (mscale_all_dim folded in) against the HuggingFace rotary module and attention"""
    s, model, _, _ = pinned
    table = deepseek.rope_cos_sin_table(s, "cpu")
    ours = R.from_hf(model)
    half = s.rope_head_dim // 2
    assert table.shape == (s.max_position, s.rope_head_dim) and table.dtype == torch.float32
    assert torch.allclose(table[:, :half], ours.cos, rtol=0, atol=2e-6)
    assert torch.allclose(table[:, half:], ours.sin, rtol=0, atol=2e-6)
    assert deepseek.attention_sm_scale(s) == pytest.approx(ours.cfg.mla.sm_scale, rel=1e-6)
    if s.rope_type == "yarn":
        from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
        inv, factor = ROPE_INIT_FUNCTIONS["yarn"](model.config, "cpu")
        mine, my_factor = deepseek.yarn_inv_freq(s)
        assert torch.equal(mine, inv.float()) and my_factor == pytest.approx(float(factor), rel=1e-7)
        assert my_factor != 1.0 and not torch.equal(mine, 1.0 / (s.rope_theta ** (torch.arange(0, 64, 2) / 64.0)))


@pytest.mark.parametrize("q_lora_rank", (None, 64))
@pytest.mark.parametrize("interleaved", (True, False))
def test_absorbed_form_is_the_naive_form_in_float64(q_lora_rank, interleaved):
    cfg = R.MLAConfig(n_heads=4, nope=32, rope=64, v_dim=32, latent=128, q_lora_rank=q_lora_rank,
                      interleaved=interleaved)
    W = R.random_mla_weights(cfg, 256, seed=1, dtype=torch.float64)
    x = torch.randn(19, 256, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    cos, sin = R.default_cos_sin(19, 64, dtype=torch.float64)
    naive, absorbed = R.mla_naive(x, W, cfg, cos, sin), R.mla_absorbed(x, W, cfg, cos, sin)
    assert rel_l2(absorbed.numpy(), naive.numpy()) < 1e-13
    # the identity is about W_UK and W_UV: exchanging two heads' value projections is seen
    assert rel_l2(R.mla_naive(x, W, cfg, cos, sin, swap_uv=(0, 1)).numpy(), naive.numpy()) > 0.1
    # and the bf16 composition is close to, not equal to, the exact form
    W32 = {k: R.bf16_round(v.float()) for k, v in W.items()}
    c32, s32 = R.default_cos_sin(19, 64)
    x32 = R.bf16_round(x.float())
    e = rel_l2(R.mla_absorbed(x32, W32, cfg, c32, s32, rnd=R.bf16_round).numpy(),
               R.mla_naive(x32, W32, cfg, c32, s32).numpy().astype(np.float64))
    assert 1e-4 < e < 2e-2


def test_presets():
    t, q, v = deepseek.DeepseekV2Shape.tiny(), deepseek.DeepseekV2Shape.tiny_qlora(), deepseek.DeepseekV2Shape.v2_lite()
    assert (t.hidden, t.n_heads, t.nope_head_dim, t.rope_head_dim, t.v_head_dim, t.kv_lora_rank) == (256, 4, 32, 64, 32, 128)
    assert (t.intermediate, t.moe_intermediate, t.n_routed_experts, t.n_shared_experts, t.topk) == (512, 128, 8, 2, 3)
    assert (t.first_k_dense_replace, t.n_layers, t.vocab, t.q_lora_rank, q.q_lora_rank) == (1, 3, 1024, None, 64)
    for n in (t.hidden, t.nope_head_dim, t.v_head_dim, t.kv_lora_rank, t.moe_intermediate, 64):
        assert n % 32 == 0
    assert (v.hidden, v.n_layers, v.n_heads, v.nope_head_dim, v.rope_head_dim, v.v_head_dim, v.kv_lora_rank) == \
        (2048, 27, 16, 128, 64, 128, 512)
    assert (v.n_routed_experts, v.n_shared_experts, v.topk, v.moe_intermediate, v.intermediate) == (64, 2, 6, 1408, 10944)
    assert (v.first_k_dense_replace, v.vocab, v.rope_factor, v.rope_type) == (1, 102400, 40.0, "yarn")
    assert "UNVERIFIED" in deepseek.DeepseekV2Shape.v2_lite.__doc__


def test_the_step_refuses_what_is_out_of_scope_before_touching_a_gpu():
    from scalellm_amd.model_parallel import ParallelArgs
    s = deepseek.DeepseekV2Shape.tiny()
    mk = lambda **kw: deepseek.DeepseekV2DecodeStep(kw.pop("shape", s), 8, 4, 16, device="cpu", **kw)  # noqa: E731
    with pytest.raises(ValueError, match="one rank"):
        mk(parallel_args=ParallelArgs(rank=0, world_size=2))
    with pytest.raises(ValueError, match="one rank"):
        mk(custom_allreduce=object())
    with pytest.raises(ValueError, match="quant_method"):
        mk(quant_method="awq")
    g = deepseek.DeepseekV2Shape.tiny()
    g.topk_method = "group_limited_greedy"
    with pytest.raises(ValueError, match="group_limited_greedy"):
        mk(shape=g)
    f = deepseek.DeepseekV2Shape.tiny()
    f.routed_scaling_factor = 16.0
    with pytest.raises(ValueError, match="routed_scaling_factor"):
        mk(shape=f)
