"""CPU tests of the fused MoE router boundary (include/slm_hip.h section 17: slm_moe_router, slm_moe_router_splits,
slm_moe_router_workspace_bytes): the symbols, the ctypes mirror of the argument struct, argument validation before
any launch, the planning helpers, the layers' `router` option without a GPU, MixtralShape's presets, and the
torch-fp32 Mixtral restatement (tests/mixtral_model_ref.py) pinned on the installed HuggingFace MixtralForCausalLM."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from scalellm_amd import _lib

from . import mixtral_model_ref as R
from .e2e_common import check_logits, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")

INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT = -1, -2, -3, -5


def test_status_codes_are_the_headers():
    text = open(HEADER).read()
    for name, val in (("SLM_ERR_INVALID_ARG", INVALID), ("SLM_ERR_UNSUPPORTED", UNSUPPORTED),
                      ("SLM_ERR_WORKSPACE", WORKSPACE), ("SLM_ERR_ALIGNMENT", ALIGNMENT)):
        assert re.search(rf"{name}\s*=\s*{val}\b", text), name


def test_the_three_symbols_are_in_the_header_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"SLM_API\s+int\s+slm_moe_router\s*\(const slm_moe_router_args\*", text)
    assert re.search(r"SLM_API\s+int\s+slm_moe_router_splits\s*\(int32_t n_experts, int64_t hidden, int32_t dtype", text)
    assert re.search(r"SLM_API\s+int\s+slm_moe_router_workspace_bytes\s*\(int64_t n_tokens, int32_t n_experts", text)
    L = _lib.lib()
    for name in ("slm_moe_router", "slm_moe_router_splits", "slm_moe_router_workspace_bytes"):
        fn = getattr(L, name)                            # AttributeError: not exported
        assert fn.argtypes is not None, name             # resolved by _lib with a prototype
    assert L.slm_moe_router.argtypes[0]._type_ is _lib.MoeRouterArgs
    from scalellm_amd import kernels
    assert callable(kernels.moe_router) and callable(kernels.moe_router_splits)


def test_router_struct_matches_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cname, cls = "slm_moe_router_args", _lib.MoeRouterArgs
    assert [f for f, _ in cls._fields_] == [
        "x", "gate_w", "correction_bias", "weights", "indices", "logits_out", "workspace", "workspace_bytes",
        "n_tokens", "hidden", "ldx", "ldw", "n_experts", "topk", "dtype", "scoring", "renormalize", "n_expert_groups",
        "topk_group", "scaling_factor"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             f'  printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out.pop("size")) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(out[fname]) == getattr(cls, fname).offset, fname


H0, E0 = 256, 8


def _args(**kw):
    a = _lib.MoeRouterArgs()
    a.x = a.gate_w = a.correction_bias = a.weights = a.indices = a.logits_out = 4096       # never touched
    a.n_tokens, a.hidden, a.ldx, a.ldw = 5, H0, H0, H0
    a.n_experts, a.topk, a.dtype, a.scoring, a.renormalize = E0, 2, _lib.SLM_BF16, 0, 1
    a.n_expert_groups, a.topk_group, a.scaling_factor = 4, 2, 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_router_validation_precedes_any_launch():
    G = _lib.lib().slm_moe_router
    rc = lambda **kw: G(C.byref(_args(**kw)), None)  # noqa: E731
    assert G(None, None) == INVALID
    # NULL or negative arguments
    for kw in (dict(n_tokens=-1), dict(hidden=0), dict(hidden=-32), dict(n_experts=0), dict(topk=0), dict(topk=E0 + 1),
               dict(workspace_bytes=-1), dict(scoring=2), dict(scoring=-1)):
        assert rc(**kw) == INVALID, kw
    for ptr in ("x", "gate_w", "weights", "indices"):
        assert rc(**{ptr: None}) == INVALID, ptr
    assert rc(logits_out=None) != INVALID and rc(correction_bias=None) != INVALID       # both optional with scoring 0
    # a stride below its extent
    assert rc(ldx=H0 - 8) == INVALID
    assert rc(ldw=H0 - 8) == INVALID
    # the grouped form: the bias is required, and section 10's conditions hold
    assert rc(scoring=1, correction_bias=None) == INVALID
    for kw in (dict(n_expert_groups=0), dict(n_expert_groups=3), dict(n_expert_groups=8), dict(topk_group=0),
               dict(topk_group=5), dict(topk=5)):                                        # 5 > topk_group * group size
        assert rc(scoring=1, **kw) == INVALID, kw
    # dtype, E or hidden outside the limits
    assert rc(dtype=_lib.SLM_F32) == UNSUPPORTED
    assert rc(n_experts=12) == UNSUPPORTED                                               # not a power of two
    assert rc(n_experts=512, topk=2) == UNSUPPORTED                                      # above section 10's limit
    assert rc(hidden=H0 + 16, ldx=H0 + 16, ldw=H0 + 16) == UNSUPPORTED                   # hidden % 32
    # misaligned pointers or strides (16-byte loads of x and the gate; fp32 / int32 outputs)
    assert rc(x=4096 + 8) == ALIGNMENT
    assert rc(gate_w=4096 + 8) == ALIGNMENT
    assert rc(ldx=H0 + 4) == ALIGNMENT
    assert rc(ldw=H0 + 4) == ALIGNMENT
    assert rc(weights=4098) == ALIGNMENT
    assert rc(indices=4098) == ALIGNMENT
    assert rc(logits_out=4098) == ALIGNMENT
    assert rc(scoring=1, correction_bias=4098) == ALIGNMENT
    # no tokens: a no-op, whatever the pointers
    assert rc(n_tokens=0, x=None, weights=None, indices=None) == 0
    assert rc(n_tokens=0, scoring=1, correction_bias=None) == 0


def test_splits_do_not_take_the_token_count_and_are_stable():
    L = _lib.lib()
    assert len(L.slm_moe_router_splits.argtypes) == 4                                    # (E, hidden, dtype, *splits)
    seen = {}
    for E, H in ((8, 4096), (64, 512), (256, 7168), (1, 32), (256, 32)):
        for dt in (_lib.SLM_BF16, _lib.SLM_F16):
            s = C.c_int32(-1)
            assert L.slm_moe_router_splits(E, H, dt, C.byref(s)) == 0
            assert s.value >= 1
            seen[(E, H, dt)] = s.value
            s2 = C.c_int32(-1)
            assert L.slm_moe_router_splits(E, H, dt, C.byref(s2)) == 0 and s2.value == s.value
            for T in (0, 1, 32, 33, 4096):
                b = C.c_size_t(123)
                assert L.slm_moe_router_workspace_bytes(T, E, H, dt, C.byref(b)) == 0
                if s.value == 1:
                    assert b.value == 0, (T, E, H)                                       # one slice: no workspace
    s = C.c_int32(0)
    assert L.slm_moe_router_splits(8, 4096, _lib.SLM_BF16, None) == INVALID
    assert L.slm_moe_router_splits(0, 4096, _lib.SLM_BF16, C.byref(s)) == INVALID
    assert L.slm_moe_router_splits(12, 4096, _lib.SLM_BF16, C.byref(s)) == UNSUPPORTED
    assert L.slm_moe_router_splits(8, 4100, _lib.SLM_BF16, C.byref(s)) == UNSUPPORTED
    assert L.slm_moe_router_splits(8, 4096, _lib.SLM_F32, C.byref(s)) == UNSUPPORTED
    b = C.c_size_t(0)
    assert L.slm_moe_router_workspace_bytes(-1, 8, 4096, _lib.SLM_BF16, C.byref(b)) == INVALID
    assert L.slm_moe_router_workspace_bytes(1, 8, 4096, _lib.SLM_BF16, None) == INVALID
    from scalellm_amd import kernels
    assert kernels.moe_router_splits(8, 4096, torch.bfloat16) == seen[(8, 4096, _lib.SLM_BF16)]
    with pytest.raises(kernels.SlmError):
        kernels.moe_router_splits(8, 4096, torch.float32)


def test_the_router_needs_gpu_tensors():
    from scalellm_amd import kernels
    x, w = torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(8, 64, dtype=torch.bfloat16)
    with pytest.raises(kernels.SlmError):
        kernels.moe_router(x, w, 2)


# ---- the layers' router option ---------------------------------------------------------------------------------------
def test_layers_take_router_torch_or_fused_and_nothing_else():
    from scalellm_amd import moe
    from scalellm_amd.kernels import SlmError
    H, I, E = 64, 96, 4
    pg = types.SimpleNamespace(world_size=2, rank=1)
    with pytest.raises(SlmError):
        moe.FusedMoE(H, I, E, 2, device="cpu", router="nonsense")
    with pytest.raises(SlmError):
        moe.ExpertParallelMoE(H, I, E, 2, pg, device="cpu", router="nonsense")
    default, torch_ = moe.FusedMoE(H, I, E, 2, device="cpu"), moe.FusedMoE(H, I, E, 2, device="cpu", router="torch")
    fused = moe.FusedMoE(H, I, E, 2, device="cpu", router="fused")
    assert (default.router, torch_.router, fused.router) == ("torch", "torch", "fused")
    assert moe.ExpertParallelMoE(H, I, E, 2, pg, device="cpu").router == "torch"
    assert moe.ExpertParallelMoE(H, I, E, 2, pg, device="cpu", router="fused").router == "fused"
    # router="torch" builds exactly what the layer built before the option existed
    keys = lambda o: sorted(k for k in vars(o) if k != "router")  # noqa: E731
    assert keys(default) == keys(torch_) == keys(fused) == sorted(
        ["hidden", "intermediate", "n_experts", "topk", "scoring", "renormalize", "n_expert_groups", "topk_group",
         "scaling_factor", "max_tokens", "dtype", "device", "experts", "gate_weight", "correction_bias", "_gate_f32_t",
         "_buf"])
    for a in ("scoring", "renormalize", "n_expert_groups", "topk_group", "scaling_factor", "max_tokens", "dtype"):
        assert getattr(default, a) == getattr(torch_, a), a
    assert type(default.experts) is type(torch_.experts) is moe.MoEDenseExperts
    sd = {"gate.weight": torch.randn(E, H).to(torch.bfloat16)}
    torch_.load_state_dict(sd)
    assert torch_._gate_f32_t is None and torch.equal(torch_.gate_weight, sd["gate.weight"])


# ---- MixtralShape -------------------------------------------------------------------------------------------------------
def test_mixtral_8x7b_preset_is_the_installed_mixtral_config():
    transformers = pytest.importorskip("transformers")
    from scalellm_amd.mixtral import MixtralShape
    cfg, s = transformers.MixtralConfig(), MixtralShape.mixtral_8x7b()
    rope_theta = getattr(cfg, "rope_theta", None) or (getattr(cfg, "rope_parameters", None) or {}).get("rope_theta")
    head_dim = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
    want = dict(hidden=cfg.hidden_size, n_heads=cfg.num_attention_heads, n_kv_heads=cfg.num_key_value_heads,
                head_dim=head_dim, intermediate=cfg.intermediate_size, n_layers=cfg.num_hidden_layers,
                vocab=cfg.vocab_size, rope_theta=float(rope_theta), rms_eps=cfg.rms_norm_eps,
                max_position=cfg.max_position_embeddings, n_experts=cfg.num_local_experts,
                topk=cfg.num_experts_per_tok)
    assert dataclasses.asdict(s) == want
    assert want == dict(hidden=4096, n_heads=32, n_kv_heads=8, head_dim=128, intermediate=14336, n_layers=32,
                        vocab=32000, rope_theta=1e6, rms_eps=1e-5, max_position=131072, n_experts=8, topk=2)
    assert not cfg.tie_word_embeddings                                                   # an untied lm_head
    big, tiny = MixtralShape.mixtral_8x22b(), MixtralShape.tiny()
    assert (big.hidden, big.n_heads, big.n_kv_heads, big.head_dim, big.intermediate, big.n_layers, big.vocab,
            big.rope_theta, big.rms_eps, big.max_position, big.n_experts, big.topk) == \
        (6144, 48, 8, 128, 16384, 56, 32000, 1e6, 1e-5, 65536, 8, 2)
    assert "UNVERIFIED" in MixtralShape.mixtral_8x22b.__doc__
    assert (tiny.hidden, tiny.n_heads, tiny.n_kv_heads, tiny.head_dim, tiny.intermediate, tiny.n_layers, tiny.vocab,
            tiny.n_experts, tiny.topk) == (256, 8, 2, 32, 512, 2, 1024, 8, 2)
    assert tiny.hidden % 128 == 0 and tiny.intermediate % 128 == 0                       # int4: K % 128, N % 64


def test_mixtral_step_refuses_more_than_one_rank_before_touching_a_gpu():
    from scalellm_amd.mixtral import MixtralDecodeStep, MixtralShape
    from scalellm_amd.model_parallel import ParallelArgs
    with pytest.raises(ValueError, match="one rank"):
        MixtralDecodeStep(MixtralShape.tiny(), 8, 4, 16, parallel_args=ParallelArgs(rank=0, world_size=2))
    with pytest.raises(ValueError):
        MixtralDecodeStep(MixtralShape.tiny(), 8, 4, 16, quant_method="gptq8")


# ---- the restatement, pinned on HuggingFace ---------------------------------------------------------------------------
TOL = 1e-4                           # the Llama and Gemma-2 pins' bound: torch's fp32 noise
SEQ_LEN = 24


@pytest.fixture(scope="module")
def pinned():
    transformers = pytest.importorskip("transformers")
    mm = pytest.importorskip("transformers.models.mixtral.modeling_mixtral")
    cfg = transformers.MixtralConfig(
        hidden_size=64, num_attention_heads=4, num_key_value_heads=2, head_dim=16, intermediate_size=96,
        num_hidden_layers=2, vocab_size=128, num_local_experts=4, num_experts_per_tok=2, max_position_embeddings=128,
        rms_norm_eps=1e-5, attention_dropout=0.0, sliding_window=None, tie_word_embeddings=False,
        router_jitter_noise=0.0)
    cfg._attn_implementation = "eager"
    torch.manual_seed(7)
    model = mm.MixtralForCausalLM(cfg).eval().float()
    with torch.no_grad():                                          # make every term matter
        for name, p in model.named_parameters():
            if name.endswith("norm.weight") or "layernorm" in name:
                p.copy_(1 + 0.3 * torch.randn_like(p))
            elif "gate.weight" in name:
                p.copy_(0.5 * torch.randn_like(p))
            else:
                p.copy_(0.1 * torch.randn_like(p))
    tokens = torch.from_numpy(np.random.default_rng(11).integers(0, 128, size=SEQ_LEN))
    with torch.no_grad():
        ref = model(input_ids=tokens[None]).logits[0].float().numpy()
    return model, ref, tokens


def test_restatement_matches_hf_mixtral(pinned):
    model, ref, tokens = pinned
    ours = R.from_hf(model)
    assert ours.cfg.topk == 2 and ours.layers[0]["gate"].shape == (4, 64) and ours.layers[0]["w1"].shape == (4, 96, 64)
    got, router = ours.logits(tokens, return_router=True)
    same, n, rel = check_logits(got.numpy(), ref, TOL, "restatement vs HF MixtralForCausalLM")
    print(f"\n[mixtral-ref] rel L2 {rel:.2e}, greedy ids equal in {same} of {n} rows")
    assert len(router) == 2 and router[0].shape == (SEQ_LEN, 4)
    # forcing the model's own selection changes nothing
    own = [R.free_topk(r, 2) for r in router]
    assert torch.equal(ours.logits(tokens, forced=own), got)


def test_every_moe_term_is_pinned_too(pinned):
    """no renormalisation, another k, the selection rotated by one expert, w1 and w3 swapped: each moves the logits
    past the bound, so the pin above holds each of them in place"""
    model, ref, tokens = pinned
    ours = R.from_hf(model)
    _, router = ours.logits(tokens, return_router=True)
    own = [R.free_topk(r, 2) for r in router]
    assert rel_l2(ours.variant(renormalize=False).logits(tokens).numpy(), ref) > 10 * TOL
    assert rel_l2(ours.variant(topk=1).logits(tokens).numpy(), ref) > 10 * TOL
    assert rel_l2(ours.logits(tokens, forced=[(s + 1) % 4 for s in own]).numpy(), ref) > 10 * TOL
    swapped = [dict(W, w1=W["w3"], w3=W["w1"]) for W in ours.layers]
    assert rel_l2(R.MixtralRef(swapped, ours.final_norm, ours.embed, ours.lm_head, ours.cfg).logits(tokens).numpy(),
                  ref) > 10 * TOL
