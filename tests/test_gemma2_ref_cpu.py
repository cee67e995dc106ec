"""tests/gemma2_model_ref.py (the reference of the Gemma-2 step's GPU test) pinned on HuggingFace Gemma2ForCausalLM
(eager attention, fp32) on the tiny configuration the GPU test uses: logits within the relative-L2 bound of the
Llama pin (tests/test_e2e_oracle_cpu.py: check_logits at 1e-4), greedy ids by check_logits' margin rule.

HF counts the window differently from the reference: HF's sliding_window is the number of keys a query sees, itself
included; the reference's W (key j visible when 0 <= i - j <= W) is the number of keys behind it.  So the reference's
W is HF's sliding_window - 1: asserted here, and the neighbouring values are asserted to FAIL."""
import numpy as np
import pytest
import torch

from tests import gemma2_model_ref as R
from tests.e2e_common import check_logits, rel_l2

transformers = pytest.importorskip("transformers")
mg = pytest.importorskip("transformers.models.gemma2.modeling_gemma2")

TOL = 1e-4                           # the Llama pin's bound (tests/test_e2e_oracle_cpu.py)
W = 16                               # the reference's window of the tiny configuration
SEQ_LEN = 40                         # kv crosses W + 1


def _hf_model(sliding_window):
    cfg = transformers.Gemma2Config(
        hidden_size=512, num_attention_heads=2, num_key_value_heads=1, head_dim=256, intermediate_size=1024,
        num_hidden_layers=4, vocab_size=1024, max_position_embeddings=512, rms_norm_eps=1e-6,
        query_pre_attn_scalar=144, sliding_window=sliding_window, attn_logit_softcapping=50.0,
        final_logit_softcapping=30.0, hidden_activation="gelu_pytorch_tanh", attention_dropout=0.0,
        tie_word_embeddings=True)
    cfg._attn_implementation = "eager"
    torch.manual_seed(5)
    model = mg.Gemma2ForCausalLM(cfg).eval().float()
    with torch.no_grad():                                          # HF initialises norm weights to 0 and the
        for name, p in model.named_parameters():                   # embedding small: make every term matter
            if name.endswith("norm.weight") or "layernorm" in name:
                p.copy_(0.3 * torch.randn_like(p))
            elif "embed_tokens" in name:
                p.copy_(0.05 * torch.randn_like(p))
            else:
                p.copy_(0.06 * torch.randn_like(p))
    return model


@pytest.fixture(scope="module")
def pinned():
    """(HF model at sliding_window = W + 1, its logits on the test sequence, the tokens)"""
    model = _hf_model(W + 1)
    tokens = torch.from_numpy(np.random.default_rng(11).integers(0, 1024, size=SEQ_LEN))
    with torch.no_grad():
        ref = model(input_ids=tokens[None]).logits[0].float().numpy()
    return model, ref, tokens


def test_layer_pattern_is_sliding_on_even_layers(pinned):
    model = pinned[0]
    types = list(model.config.layer_types)
    assert types == ["sliding_attention", "full_attention"] * 2     # gemma2.h:249-251: (i % 2) == 0 slides


def test_restatement_matches_hf_gemma2(pinned):
    model, ref, tokens = pinned
    ours = R.from_hf(model)
    assert ours.cfg.sliding_window == W and ours.cfg.attn_scalar == 144 != ours.cfg.head_dim
    got = ours.logits(tokens).numpy()
    same, n, rel = check_logits(got, ref, TOL, "restatement vs HF Gemma2ForCausalLM")
    print(f"\n[gemma2-ref] rel L2 {rel:.2e}, greedy ids equal in {same} of {n} rows")
    assert np.abs(got).max() <= 30.0 and np.abs(ref).max() <= 30.0
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("w_ref", [W - 1, W + 1])
def test_the_neighbouring_window_fails(pinned, w_ref):
    """the reference's W is HF's sliding_window - 1 and nothing else: one key more or less exceeds the bound"""
    model, ref, tokens = pinned
    got = R.from_hf(model).variant(sliding_window=w_ref).logits(tokens).numpy()
    np.testing.assert_allclose(got[:W], ref[:W], rtol=2e-4, atol=2e-4)   # rows that see every key either way
    assert rel_l2(got, ref) > 10 * TOL


def test_every_other_term_is_pinned_too(pinned):
    """window off, sm_scale from head_dim, no attention cap, the T-rounded embedding scale of a bf16 model: each
    moves the logits past the bound, so the pin above holds each of them in place"""
    model, ref, tokens = pinned
    ours = R.from_hf(model)
    bf16_scale = float(torch.tensor(512.0 ** 0.5, dtype=torch.bfloat16).float())
    for change in (dict(sliding_window=-1), dict(sm_scale=256.0 ** -0.5), dict(attn_logit_soft_cap=0.0),
                   dict(final_logit_soft_cap=60.0), dict(embed_scale=bf16_scale * 1.01)):
        assert rel_l2(ours.variant(**change).logits(tokens).numpy(), ref) > 10 * TOL, change
