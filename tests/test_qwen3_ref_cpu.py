"""CPU tests of the Qwen3 family: the shape presets, the step's refusals before any GPU work, and the torch-fp32
restatement (tests/qwen3_model_ref.py) pinned on the installed HuggingFace Qwen3ForCausalLM and Qwen3MoeForCausalLM
built from tiny configurations (dense and MoE, tied and untied head) with the same weights."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import qwen3_model_ref as R
from tests.e2e_common import check_logits, rel_l2

TOL = 1e-4                           # the Llama, Gemma-2, Mixtral and DeepSeek pins' bound: torch's fp32 noise
SEQ_LEN = 24


# ---- Qwen3Shape ---------------------------------------------------------------------------------------------------
def test_presets():
    from scalellm_amd.qwen3 import Qwen3Shape
    fields = [f.name for f in dataclasses.fields(Qwen3Shape)]
    assert fields == ["hidden", "n_heads", "n_kv_heads", "head_dim", "intermediate", "n_layers", "vocab", "rope_theta",
                      "rms_eps", "max_position", "tie_word_embeddings", "n_experts", "topk", "moe_intermediate",
                      "norm_topk_prob"]
    # no config.json of either checkpoint is at hand to compare field by field: both say so
    for preset in (Qwen3Shape.qwen3_8b, Qwen3Shape.qwen3_30b_a3b):
        assert "UNVERIFIED" in preset.__doc__
    s8, s30 = Qwen3Shape.qwen3_8b(), Qwen3Shape.qwen3_30b_a3b()
    assert (s8.hidden, s8.n_heads, s8.n_kv_heads, s8.head_dim, s8.n_experts) == (4096, 32, 8, 128, 0)
    assert (s30.hidden, s30.n_kv_heads, s30.n_experts, s30.topk, s30.moe_intermediate) == (2048, 4, 128, 8, 768)
    for s in (Qwen3Shape.tiny(), Qwen3Shape.tiny_moe()):
        assert s.n_heads * s.head_dim != s.hidden and s.head_dim in (64, 128, 256)
        assert s.hidden % 128 == 0 and s.intermediate % 128 == 0 and (s.n_heads * s.head_dim) % 128 == 0
    m = Qwen3Shape.tiny_moe()
    assert (m.n_experts, m.topk, m.moe_intermediate) == (8, 2, 128) and m.moe_intermediate % 128 == 0


def test_the_step_refuses_what_is_out_of_scope_before_touching_a_gpu():
    from scalellm_amd.model_parallel import ParallelArgs
    from scalellm_amd.qwen3 import Qwen3DecodeStep, Qwen3Shape
    with pytest.raises(ValueError, match="one rank"):
        Qwen3DecodeStep(Qwen3Shape.tiny(), 8, 4, 16, parallel_args=ParallelArgs(rank=0, world_size=2))
    with pytest.raises(ValueError):
        Qwen3DecodeStep(Qwen3Shape.tiny(), 8, 4, 16, quant_method="gptq8")
    with pytest.raises(ValueError, match="head_dim"):
        Qwen3DecodeStep(dataclasses.replace(Qwen3Shape.tiny(), head_dim=32), 8, 4, 16)
    with pytest.raises(ValueError, match="record_routing"):
        Qwen3DecodeStep(Qwen3Shape.tiny(), 8, 4, 16, record_routing=True)


def test_the_handler_takes_both_norm_weights_or_neither():
    from scalellm_amd import kernels
    from scalellm_amd.layers import HipAttnHandler
    w, cs = torch.ones(64), torch.zeros(8, 64)
    with pytest.raises(kernels.SlmError):
        HipAttnHandler(1.0, rotary_dim=64, cos_sin=cs, q_norm=w)
    with pytest.raises(kernels.SlmError):
        HipAttnHandler(1.0, rotary_dim=64, cos_sin=cs, q_norm=w, k_norm=w)          # no eps
    with pytest.raises(kernels.SlmError):
        HipAttnHandler(1.0, q_norm=w, k_norm=w, qk_norm_eps=1e-6)                    # no RoPE
    h = HipAttnHandler(1.0, rotary_dim=64, cos_sin=cs)
    assert h.q_norm is None and h.k_norm is None                                     # the old path, unchanged


# ---- the restatement, pinned on HuggingFace -----------------------------------------------------------------------
def _build(moe, tied):
    transformers = pytest.importorskip("transformers")
    common = dict(hidden_size=64, num_attention_heads=4, num_key_value_heads=2, head_dim=32, num_hidden_layers=2,
                  vocab_size=128, max_position_embeddings=128, rms_norm_eps=1e-6, attention_dropout=0.0,
                  tie_word_embeddings=tied, rope_parameters={"rope_type": "default", "rope_theta": 1e6})
    if moe:
        mm = pytest.importorskip("transformers.models.qwen3_moe.modeling_qwen3_moe")
        cfg = transformers.Qwen3MoeConfig(intermediate_size=96, moe_intermediate_size=48, num_experts=4,
                                          num_experts_per_tok=2, norm_topk_prob=True, decoder_sparse_step=1,
                                          mlp_only_layers=[], **common)
        cls = mm.Qwen3MoeForCausalLM
    else:
        mm = pytest.importorskip("transformers.models.qwen3.modeling_qwen3")
        cfg = transformers.Qwen3Config(intermediate_size=96, **common)
        cls = mm.Qwen3ForCausalLM
    cfg._attn_implementation = "eager"
    torch.manual_seed(7)
    model = cls(cfg).eval().float()
    with torch.no_grad():                                          # make every term matter
        for name, p in model.named_parameters():
            if "norm" in name:
                p.copy_(1 + 0.3 * torch.randn_like(p))
            elif "gate.weight" in name:
                p.copy_(0.5 * torch.randn_like(p))
            else:
                p.copy_(0.1 * torch.randn_like(p))
    if tied:
        assert model.lm_head.weight.data_ptr() == model.model.embed_tokens.weight.data_ptr()
    tokens = torch.from_numpy(np.random.default_rng(11).integers(0, 128, size=SEQ_LEN))
    with torch.no_grad():
        ref = model(input_ids=tokens[None]).logits[0].float().numpy()
    return model, ref, tokens


@pytest.fixture(scope="module", params=[(False, False), (False, True), (True, False)],
                ids=["dense", "dense-tied", "moe"])
def pinned(request):
    moe, tied = request.param
    return (moe, tied) + _build(moe, tied)


def test_restatement_matches_hf_qwen3(pinned):
    moe, tied, model, ref, tokens = pinned
    ours = R.from_hf(model)
    assert ours.cfg.n_experts == (4 if moe else 0) and ours.layers[0]["q_norm"].shape == (32,)
    got = ours.logits(tokens)
    same, n, rel = check_logits(got.numpy(), ref, TOL, f"restatement vs HF (moe {moe}, tied {tied})")
    print(f"\n[qwen3-ref] moe {moe} tied {tied}: rel L2 {rel:.2e}, greedy ids equal in {same} of {n} rows")
    if moe:                                                        # forcing the model's own selection changes nothing
        _, router = ours.logits(tokens, return_router=True)
        own = [R.free_topk(r, 2) for r in router]
        assert torch.equal(ours.logits(tokens, forced=own), got)


def test_every_qwen3_term_is_pinned_too(pinned):
    """without q_norm / k_norm, with q_norm and k_norm swapped, and (MoE) without the renormalisation or with the
    selection rotated by one expert: each moves the logits past the bound, so the pin holds each of them in place"""
    moe, _, model, ref, tokens = pinned
    ours = R.from_hf(model)
    assert rel_l2(ours.variant(qk_norm=False).logits(tokens).numpy(), ref) > 10 * TOL
    swapped = [dict(W, q_norm=W["k_norm"], k_norm=W["q_norm"]) for W in ours.layers]
    assert rel_l2(R.Qwen3Ref(swapped, ours.final_norm, ours.embed, ours.lm_head, ours.cfg).logits(tokens).numpy(),
                  ref) > 10 * TOL
    if moe:
        _, router = ours.logits(tokens, return_router=True)
        own = [R.free_topk(r, 2) for r in router]
        assert rel_l2(ours.variant(renormalize=False).logits(tokens).numpy(), ref) > 10 * TOL
        assert rel_l2(ours.logits(tokens, forced=[(s + 1) % 4 for s in own]).numpy(), ref) > 10 * TOL
