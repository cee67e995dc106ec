"""CPU checks of tests/gemma_ref.py and of the two Gemma entry points' argument validation (no GPU):
the float64 GN is the reference's detail::gemma_rms_norm and HF's Gemma2RMSNorm, an fp32 restatement of the kernel
arithmetic stays below HALF of every cap with its rsqrt off by 0 and +-8 fp32 ulps, each plausible wrong kernel
breaks a cap at least tenfold, every invalid argument returns its code before any launch, and the ctypes struct
matches the header."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from scalellm_amd import _lib
from scalellm_amd._lib import GemmaNormArgs
from tests import gemma_ref as G
from tests import helpers
from tests.glue_ref import BITS, f64_to_t_bits, round_to_t, t_bits_to_f64, t_ulp_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_T = {"bf16": torch.bfloat16, "f16": torch.float16}
RESTATEMENT_CASES = [(8, 512), (2304, 4), (4608, 4)]   # tokens * dim >= 4096 each
RS_ULPS = (0, 8, -8)


def _torch_t(a, bits):
    return torch.from_numpy(np.array(a, np.float64)).to(TORCH_T[bits])


def _bits_of(t, bits):
    return helpers._t_bits(t.float().numpy(), bits)


def _share_dist(got, want):
    d = t_ulp_distance(got, want)
    return float((d != 0).mean()), int(d.max())


# ---- the reference is the reference's ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_f64_gn_is_the_reference_gemma_rms_norm_in_torch_fp32(bits):
    """detail::gemma_rms_norm (normalization.h:31-40) restated in torch: fp32 norm, * (1 + w.float()), one cast"""
    x, _, pre, _ = G.norm_inputs(bits, 2304, 4)
    xt, wt = _torch_t(x, bits), _torch_t(pre, bits)
    xf = xt.float()
    out = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + G.GEMMA_EPS) * (1.0 + wt.float())).to(xt.dtype)
    share, dist = _share_dist(_bits_of(out, bits), G.gn_ref(x, pre, bits=bits))
    assert dist <= G.OUT_CAP[1] and share <= G.OUT_CAP[0] / 2, (share, dist)


@pytest.mark.parametrize("bits", BITS)
def test_f64_gn_is_hf_gemma2_rms_norm(bits):
    m = pytest.importorskip("transformers.models.gemma2.modeling_gemma2")
    x, _, pre, _ = G.norm_inputs(bits, 2304, 4)
    norm = m.Gemma2RMSNorm(2304, eps=G.GEMMA_EPS)
    with torch.no_grad():
        norm.weight.copy_(_torch_t(pre, bits).float())
        out = norm(_torch_t(x, bits))
    assert out.dtype == TORCH_T[bits]
    share, dist = _share_dist(_bits_of(out, bits), G.gn_ref(x, pre, bits=bits))
    assert dist <= G.OUT_CAP[1] and share <= G.OUT_CAP[0] / 2, (share, dist)


# ---- the caps are attainable: fp32 arithmetic stays below half of them ------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_fp32_restatement_stays_below_half_of_every_cap(bits):
    worst = {"out": (0.0, 0), "residual": (0.0, 0)}
    for dim, tokens in RESTATEMENT_CASES:
        c = G.norm_case(bits, dim, tokens)
        for ulps in RS_ULPS:
            out, r = G.form_b_fp32(c["x"], c["post"], c["res"], c["pre"], rs_ulps=ulps, bits=bits)
            s, d = G.check_out(out, r, c["pre"], (dim, ulps), bits=bits, cap=(G.OUT_CAP[0] / 2, G.OUT_CAP[1]))
            worst["out"] = (max(worst["out"][0], s), max(worst["out"][1], d))
            exact, explained = G.residual_b_explained(r, c["y_b"], c["res"], bits=bits)
            assert explained.all(), (dim, ulps)
            worst["residual"] = (max(worst["residual"][0], float((~exact).mean())), 0)
            a = G.gn_fp32_bits(c["x"], c["pre"], rs_ulps=ulps, bits=bits)
            s, d = G.check_out(a, f64_to_t_bits(c["x"], bits), c["pre"], (dim, ulps, "A"), bits=bits,
                               cap=(G.OUT_CAP[0] / 2, G.OUT_CAP[1]))
            worst["out"] = (max(worst["out"][0], s), max(worst["out"][1], d))
    print("fp32 restatement", bits, worst)
    assert worst["residual"][0] <= G.NEIGHBOUR_CAP / 2, worst


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("cap", G.SOFT_CAPS)
def test_fp32_soft_cap_restatement_stays_below_half_of_the_cap(bits, cap):
    x, want, n_planted = G.soft_cap_case(bits, cap)
    got = G.soft_cap_fp32_bits(x, cap, bits=bits)
    share, dist = _share_dist(got, want)
    assert dist <= G.SOFT_CAP_CAP[1] and share <= G.SOFT_CAP_CAP[0] / 2, (share, dist)
    assert not t_ulp_distance(got[0, :n_planted], want[0, :n_planted]).any()   # the planted arguments: exact
    # and every |result| <= cap, the largest finite argument included
    assert np.abs(t_bits_to_f64(got, bits)).max() <= cap


# ---- the caps discriminate: wrong kernels break them at least tenfold -------------------------------------------
def _violation(out_bits, res_bits, c, bits):
    """the largest factor by which a (out, residual) pair of form B exceeds a cap: share / cap, or distance / cap"""
    want = G.gn_ref(t_bits_to_f64(res_bits, bits), c["pre"], bits=bits)
    s, d = _share_dist(out_bits, want)
    exact, explained = G.residual_b_explained(res_bits, c["y_b"], c["res"], bits=bits)
    outside = float((~explained).mean())
    # an element outside the candidates is a failure outright: count its share against the neighbour cap too
    return max(s / G.OUT_CAP[0], d / G.OUT_CAP[1], float((~exact).mean()) / G.NEIGHBOUR_CAP,
               10.0 if outside > 0 and outside * explained.size >= 10 else 0.0)


def _wrong_b(kind, c, bits):
    x, post, pre, res = c["x"], c["post"], c["pre"], c["res"]
    if kind == "llama_roundings":          # T(T(h rs) (1 + w)) in both norms
        def gn(h, w):
            h = np.asarray(h, np.float64)
            rs = 1.0 / np.sqrt((h * h).mean(-1, keepdims=True) + np.float64(np.float32(G.GEMMA_EPS)))
            return f64_to_t_bits(round_to_t(h * rs, bits) * (1.0 + w), bits)
    elif kind == "weight_without_one":
        def gn(h, w):
            return G.gn_ref(h, np.asarray(w) - 1.0, bits=bits)
    else:
        def gn(h, w):
            return G.gn_ref(h, w, bits=bits)
    if kind == "weights_swapped":
        post, pre = pre, post
    if kind == "residual_before_post_norm":
        r = f64_to_t_bits(gn_in := np.asarray(x) + np.asarray(res), bits)
        y = gn(gn_in, post)
        return gn(t_bits_to_f64(y, bits), pre), r
    y = t_bits_to_f64(gn(x, post), bits)
    r = f64_to_t_bits(y + res, bits)
    if kind == "second_norm_on_unrounded_sum":
        return gn(y + res, pre), r
    return gn(t_bits_to_f64(r, bits), pre), r


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("kind", ["llama_roundings", "weight_without_one", "second_norm_on_unrounded_sum",
                                  "residual_before_post_norm", "weights_swapped"])
def test_wrong_sandwich_kernels_break_a_cap_tenfold(bits, kind):
    c = G.norm_case(bits, 2304, 4)
    good = _violation(c["out_b"], c["res_b"], c, bits)
    assert good == 0.0
    out, r = _wrong_b(kind, c, bits)
    assert _violation(out, r, c, bits) >= 10.0, kind


@pytest.mark.parametrize("bits", BITS)
def test_a_table_row_off_by_one_breaks_form_c(bits):
    table, ids, scale, pre, out, r = G.embed_case(bits, 2304, 4)
    _, r_wrong = G.form_c_ref(table, (ids + 1) % G.VOCAB, scale, pre, bits=bits)
    assert (t_ulp_distance(r_wrong, r) != 0).mean() > 0.5     # where bit equality is owed
    # and the unscaled row, or a scale that is not a value of T, is not bit-equal either
    assert (t_ulp_distance(f64_to_t_bits(table[ids], bits), r) != 0).mean() > 0.5
    assert (t_ulp_distance(f64_to_t_bits(table[ids] * np.sqrt(2304.0), bits), r) != 0).any() or \
        G.embed_scale(2304, bits) == np.sqrt(2304.0)


def test_neighbours_step_through_zero_and_the_case_table_reaches_every_nv():
    up, down = G.t_neighbours(np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x3F80], np.uint16))
    assert up.tolist() == [0x0001, 0x0001, 0x0002, 0x0000, 0x3F81]
    assert down.tolist() == [0x8001, 0x8001, 0x0000, 0x8002, 0x3F7F]
    assert sorted({G.gemma_nv(d) for d, _ in G.CASES}) == [1, 2, 4, 8]
    for bits in BITS:                                              # the slabs' sum is exact in fp32 in any order
        slabs, x = G.slabs_case(bits, 2304, 4, 8)
        assert np.array_equal(round_to_t(slabs[::-1].sum(axis=0, dtype=np.float32).astype(np.float64), bits), x)


# ---- argument validation, before any launch (no GPU here) -------------------------------------------------------
A16 = 0x10000                        # a 16-byte aligned address that is never dereferenced: every call fails first


def _args(**kw):
    g = GemmaNormArgs()
    g.n_tokens, g.dim, g.dtype, g.eps, g.vocab, g.x_scale = 4, 64, _lib.SLM_BF16, 1e-6, 16, 8.0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


FORM_A = dict(out=A16, x=A16, pre_weight=A16)
FORM_B = dict(out=A16, x=A16, post_weight=A16, pre_weight=A16, residual=A16)
FORM_C = dict(out=A16, table=A16, token_ids=A16, pre_weight=A16, residual=A16)
PTRS = ("out", "x", "partials", "post_weight", "pre_weight", "residual", "table", "token_ids")


def _valid_form(p):
    """the form table of slm_hip.h section 12 restated over the set of non-NULL pointers (n_splits >= 1, vocab > 0)"""
    s = {k for k in PTRS if p.get(k)}
    if "table" in s:
        return s == {"table", "token_ids", "residual", "pre_weight", "out"}
    if "residual" in s:
        return ("token_ids" not in s and len(s & {"x", "partials"}) == 1 and
                ("pre_weight" in s) == ("out" in s))
    return s == {"x", "pre_weight", "out"}


def test_every_pointer_combination_outside_the_form_table_is_invalid_arg():
    """all 256 subsets of the eight pointers, with an unsupported dim: a valid form gets past the pointer check and
    fails on the dim (UNSUPPORTED), every other combination returns INVALID_ARG; nothing is launched either way"""
    L = _lib.lib()
    n_valid = 0
    for mask in range(256):
        p = {k: A16 for i, k in enumerate(PTRS) if mask >> i & 1}
        rc = L.slm_gemma_norm(C.byref(_args(dim=12, n_splits=2, **p)), None)
        assert rc == (-2 if _valid_form(p) else -1), (sorted(p), rc)
        n_valid += _valid_form(p)
    assert n_valid == 1 + 1 + 2 * 2 * 2       # A; C; B: x | partials, post or not, second stage or not
    assert L.slm_gemma_norm(None, None) == -1
    for form in (FORM_A, FORM_B, FORM_C):
        assert _valid_form(form)


def test_gemma_norm_limits_alignment_and_empty_batch():
    L = _lib.lib()
    part = {k: v for k, v in FORM_B.items() if k != "x"}
    for form in (FORM_A, FORM_B, FORM_C, dict(part, partials=A16, n_splits=4)):
        for dim in G.DIM_UNSUPPORTED:
            assert L.slm_gemma_norm(C.byref(_args(dim=dim, **form)), None) == -2, (form, dim)
        assert L.slm_gemma_norm(C.byref(_args(dtype=_lib.SLM_F32, **form)), None) == -2
        for k in form:
            if k != "n_splits":                                    # 16 bytes; the int32 ids: 4
                off = 2 if k == "token_ids" else 8
                assert L.slm_gemma_norm(C.byref(_args(**dict(form, **{k: A16 + off}))), None) == -5, k
        assert L.slm_gemma_norm(C.byref(_args(n_tokens=0, **form)), None) == 0
        assert L.slm_gemma_norm(C.byref(_args(n_tokens=-1, **form)), None) == -1
    assert L.slm_gemma_norm(C.byref(_args(partials=A16, n_splits=0, **part)), None) == -1
    assert L.slm_gemma_norm(C.byref(_args(**dict(FORM_C, vocab=0))), None) == -1


def test_soft_cap_arguments():
    L = _lib.lib()
    bf = _lib.SLM_BF16
    assert L.slm_soft_cap(None, A16, 2, 64, 30.0, bf, None) == -1
    assert L.slm_soft_cap(A16, None, 2, 64, 30.0, bf, None) == -1
    assert L.slm_soft_cap(A16, A16, -1, 64, 30.0, bf, None) == -1
    for cap in (0.0, -30.0, float("inf"), float("nan")):
        assert L.slm_soft_cap(A16, A16, 2, 64, cap, bf, None) == -1, cap
    for row_len in G.SOFT_CAP_ROW_LEN_UNSUPPORTED:
        assert L.slm_soft_cap(A16, A16, 2, row_len, 30.0, bf, None) == -2, row_len
    assert L.slm_soft_cap(A16, A16, 2, 64, 30.0, _lib.SLM_F32, None) == -2
    assert L.slm_soft_cap(A16 + 8, A16, 2, 64, 30.0, bf, None) == -5
    assert L.slm_soft_cap(A16, A16 + 2, 2, 64, 30.0, bf, None) == -5
    assert L.slm_soft_cap(A16, A16, 0, 64, 30.0, bf, None) == 0


def test_gemma_ctypes_struct_matches_the_c_header(tmp_path):
    """size and every field offset of GemmaNormArgs equal what a C compiler makes of include/slm_hip.h"""
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(slm_gemma_norm_args));']
    for fname, _ in GemmaNormArgs._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(slm_gemma_norm_args, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        field, val = line.split()
        want = C.sizeof(GemmaNormArgs) if field == "size" else getattr(GemmaNormArgs, field).offset
        assert int(val) == want, f"slm_gemma_norm_args.{field}: C says {val}, ctypes says {want}"
        seen += 1
    assert seen == len(GemmaNormArgs._fields_) + 1


def test_python_layer_and_kernel_names_exist():
    from scalellm_amd import kernels, layers
    for name in ("gemma_rms_norm", "gemma_sandwich_norm", "gemma_embed_norm", "soft_cap"):
        assert callable(getattr(kernels, name))
    assert {"load_state_dict", "verify_loaded_weights", "forward"} <= set(dir(layers.GemmaRMSNorm))
    with pytest.raises(kernels.SlmError):                          # no CPU fallback
        kernels.soft_cap(torch.zeros(2, 8, dtype=torch.bfloat16), 30.0)
