"""The references of tests/test_gemma2_decode_step_gpu.py (tests/gemma2_decode_case.py), checked without a GPU: the
fp32 forward agrees with the project's Gemma-2 restatement that is pinned on HuggingFace, the tolerances are twice
the error of the bf16 framework run, and the comparison they bound sees the sliding window and its off-by-one
neighbours."""
import torch

from tests import gemma2_decode_case as C
from tests import gemma2_model_ref as R

SD, TOKS = C.checkpoint(), C.tokens()
REF = C.decode_rows(SD, TOKS)


def _cat(new, x):
    return torch.cat([layer[x] for layer in new])


def test_fp32_reference_agrees_with_the_restatement_pinned_on_huggingface():
    c = C.HF_CONFIG
    t = lambda p, name: SD[p + name + ".weight"].float().t()  # noqa: E731
    layers = []
    for i in range(c["num_hidden_layers"]):
        p = f"model.layers.{i}."
        layers.append({
            "qkv": torch.cat([t(p, "self_attn.q_proj"), t(p, "self_attn.k_proj"), t(p, "self_attn.v_proj")], dim=1),
            "o": t(p, "self_attn.o_proj"), "gate_up": torch.cat([t(p, "mlp.gate_proj"), t(p, "mlp.up_proj")], dim=1),
            "down": t(p, "mlp.down_proj"), "in_norm": SD[p + "input_layernorm.weight"],
            "post_attn_norm": SD[p + "post_attention_layernorm.weight"],
            "pre_ffn_norm": SD[p + "pre_feedforward_layernorm.weight"],
            "post_ffn_norm": SD[p + "post_feedforward_layernorm.weight"]})
    ref = R.Gemma2Ref(layers, SD["model.norm.weight"], SD["model.embed_tokens.weight"], R.Gemma2RefConfig(
        n_heads=c["num_attention_heads"], n_kv_heads=c["num_key_value_heads"], head_dim=c["head_dim"],
        rms_eps=c["rms_norm_eps"], rope_theta=c["rope_theta"], attn_scalar=float(c["query_pre_attn_scalar"]),
        sliding_window=c["sliding_window"] - 1, attn_logit_soft_cap=c["attn_logit_softcapping"],
        final_logit_soft_cap=c["final_logit_softcapping"]))
    for s in range(C.N_SEQS):
        want = ref.logits(TOKS[s])[C.PREFILL:]
        assert C.rel_l2(REF[0][:, s], want) < 1e-5


def test_tolerances_are_twice_the_error_of_the_bf16_framework_run():
    logits, new, _ = C.decode_rows(SD, TOKS, dtype=torch.bfloat16)
    for name, err, recorded, tol in (("logits", C.rel_l2(logits, REF[0]), C.BF16_LOGITS_ERR, C.TOL_LOGITS),
                                     ("K", C.rel_l2(_cat(new, 0), _cat(REF[1], 0)), C.BF16_K_ERR, C.TOL_K),
                                     ("V", C.rel_l2(_cat(new, 1), _cat(REF[1], 1)), C.BF16_V_ERR, C.TOL_V)):
        print(f"\n[gemma2-decode-ref] {name}: bf16 run {err:.3e}, recorded {recorded:.3e}, tolerance {tol:.3e}")
        assert tol == 2 * recorded
        # (the bf16 run's rounding may differ a little between library builds: the record must stay its size)
        assert recorded / 1.25 <= err <= recorded * 1.25, name


def test_the_comparison_sees_the_window_and_its_neighbours():
    """window off, one key more and one key fewer on layer 0 all move the logits, and the K rows layer 1 appends,
    far outside the tolerances; the history is longer than the window from the first step on"""
    assert C.PREFILL + 1 > C.HF_CONFIG["sliding_window"]
    for window in (0, C.HF_CONFIG["sliding_window"] + 1, C.HF_CONFIG["sliding_window"] - 1):
        logits, new, _ = C.decode_rows(SD, TOKS, window=window)
        assert C.rel_l2(logits, REF[0]) > 4 * C.TOL_LOGITS, window
        assert C.rel_l2(new[1][0], REF[1][1][0]) > 4 * C.TOL_K, window
        assert torch.equal(new[0][0], REF[1][0][0])     # layer 0's own K does not depend on its attention


def test_shape_from_a_huggingface_config_counts_the_keys_behind_the_query():
    from scalellm_amd.gemma2 import Gemma2Shape
    s = Gemma2Shape.from_hf_config(C.HF_CONFIG)
    assert (s.hidden, s.n_heads, s.n_kv_heads, s.head_dim, s.intermediate, s.n_layers, s.vocab) == \
        (256, 2, 1, 256, 512, 2, 512)
    assert (s.attn_scalar, s.attn_logit_soft_cap, s.final_logit_soft_cap, s.rope_theta, s.rms_eps, s.max_position) == \
        (144.0, 50.0, 30.0, 10000.0, 1e-6, 128)
    assert s.sliding_window == C.HF_CONFIG["sliding_window"] - 1

    class Cfg:                                   # the object form, no window
        pass
    cfg = Cfg()
    for k, v in dict(C.HF_CONFIG, sliding_window=None).items():
        setattr(cfg, k, v)
    assert Gemma2Shape.from_hf_config(cfg).sliding_window == -1
