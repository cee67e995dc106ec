"""Bit-level tests of the Gemma kernels (csrc/gemma.hip: slm_gemma_norm forms A / B / C, slm_soft_cap) against the
float64 references and caps of tests/gemma_ref.py: every case x form x dtype through kernels.*, once through the
pybind shim; the partials form bit-equal to the x form fed with the slabs' exact sum; repeats bit-identical; the
canary intact beyond n_tokens and in a padded tail; a captured graph replayed after the inputs changed in place.
The caps are conditions (tests/test_gemma_ref_cpu.py shows an fp32 implementation meets them twice over and wrong
kernels miss them tenfold); what the device shows is printed and recorded in gemma_ref.MEASURED."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import gemma_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD_ROWS = 2                         # rows beyond n_tokens in every output buffer, filled with the canary


def _dev(vals, bits):
    """float64 values of T -> device tensor of T, through the bit patterns"""
    u = G.f64_to_t_bits(vals, bits)
    assert np.array_equal(G.t_bits_to_f64(u, bits), np.asarray(vals, np.float64)), "not values of T"
    return torch.from_numpy(u.view(np.int16).copy()).to(DEV).view(TDT[bits])


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _padded(rows, dim, bits, fill=None):
    """([rows + PAD_ROWS, dim] buffer of canaries, its first `rows` rows as a view, optionally filled)"""
    buf = torch.full((rows + PAD_ROWS, dim), G.CANARY, device=DEV, dtype=torch.int16).view(TDT[bits])
    view = buf[:rows]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _tail_intact(*bufs):
    return all((_bits(b[-PAD_ROWS:]) == G.CANARY).all() for b in bufs)


def _shim():
    path = os.path.join(ROOT, "scalellm_amd", "csrc", "_slm_shim.so")
    assert os.path.exists(path), "build it: python -m scalellm_amd.build_shim"
    spec = importlib.util.spec_from_file_location("_slm_shim", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("dim,tokens", G.CASES)
@pytest.mark.parametrize("bits", G.BITS)
def test_form_a_plain(bits, dim, tokens):
    from scalellm_amd import kernels
    c = G.norm_case(bits, dim, tokens)
    xd, wd = _dev(c["x"], bits), _dev(c["pre"], bits)
    buf, out = _padded(tokens, dim, bits)
    kernels.gemma_rms_norm(out, xd, wd, G.GEMMA_EPS)
    torch.cuda.synchronize()
    got = _bits(out)
    share, dist = G.check_out(got, G.f64_to_t_bits(c["x"], bits), c["pre"], f"A {bits} {dim}", bits=bits)
    print(f"\n[gemma-gpu] A {bits} dim {dim} NV{G.gemma_nv(dim)}: out share {share:.5f} distance {dist}")
    assert _tail_intact(buf) and np.array_equal(_bits(xd), G.f64_to_t_bits(c["x"], bits))
    kernels.gemma_rms_norm(xd, xd, wd, G.GEMMA_EPS)                # in place, and a repeat: the same bits
    torch.cuda.synchronize()
    assert np.array_equal(_bits(xd), got)


@pytest.mark.parametrize("dim,tokens", G.CASES)
@pytest.mark.parametrize("bits", G.BITS)
def test_form_b_sandwich(bits, dim, tokens):
    from scalellm_amd import kernels
    c = G.norm_case(bits, dim, tokens)
    xd, post, pre = _dev(c["x"], bits), _dev(c["post"], bits), _dev(c["pre"], bits)
    obuf, out = _padded(tokens, dim, bits)
    rbuf, res = _padded(tokens, dim, bits, _dev(c["res"], bits))
    kernels.gemma_sandwich_norm(out, xd, post, res, pre, G.GEMMA_EPS)
    torch.cuda.synchronize()
    got, got_r = _bits(out), _bits(res)
    r_share, outside = G.check_residual_b(got_r, c["y_b"], c["res"], f"B residual {bits} {dim}", bits=bits)
    share, dist = G.check_out(got, got_r, c["pre"], f"B out {bits} {dim}", bits=bits)
    print(f"\n[gemma-gpu] B {bits} dim {dim} NV{G.gemma_nv(dim)}: out share {share:.5f} distance {dist}; "
          f"residual neighbour share {r_share:.5f} outside {outside}")
    assert _tail_intact(obuf, rbuf) and np.array_equal(_bits(xd), G.f64_to_t_bits(c["x"], bits))
    # a repeat on fresh buffers: bit-identical
    obuf2, out2 = _padded(tokens, dim, bits)
    rbuf2, res2 = _padded(tokens, dim, bits, _dev(c["res"], bits))
    kernels.gemma_sandwich_norm(out2, xd, post, res2, pre, G.GEMMA_EPS)
    # no second stage: the same residual, out never touched
    rbuf3, res3 = _padded(tokens, dim, bits, _dev(c["res"], bits))
    kernels.gemma_sandwich_norm(None, xd, post, res3, None, G.GEMMA_EPS)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out2), got) and np.array_equal(_bits(res2), got_r)
    assert np.array_equal(_bits(res3), got_r) and _tail_intact(rbuf3)


@pytest.mark.parametrize("dim,tokens", [G.CASES[0], G.CASES[2], G.CASES[4]])
@pytest.mark.parametrize("bits", G.BITS)
def test_form_b_without_post_weight_is_the_plain_residual_layer(bits, dim, tokens):
    """post_weight NULL: y = x, residual = T(x + residual) bit for bit (one rounding of an fp32 sum of two T values)"""
    from scalellm_amd import kernels
    c = G.norm_case(bits, dim, tokens)
    want_out, want_r, _ = G.form_b_ref(c["x"], None, c["res"], c["pre"], bits=bits)
    obuf, out = _padded(tokens, dim, bits)
    rbuf, res = _padded(tokens, dim, bits, _dev(c["res"], bits))
    kernels.gemma_sandwich_norm(out, _dev(c["x"], bits), None, res, _dev(c["pre"], bits), G.GEMMA_EPS)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(res), want_r)
    G.check_out(_bits(out), want_r, c["pre"], f"B no post {bits} {dim}", bits=bits)
    assert _tail_intact(obuf, rbuf)


@pytest.mark.parametrize("n_splits", G.SPLITS)
@pytest.mark.parametrize("dim,tokens", G.CASES)
@pytest.mark.parametrize("bits", G.BITS)
def test_form_b_partials_equal_the_x_form_on_the_exact_sum(bits, dim, tokens, n_splits):
    from scalellm_amd import kernels
    c = G.norm_case(bits, dim, tokens)
    slabs, x = G.slabs_case(bits, dim, tokens, n_splits)
    post, pre = _dev(c["post"], bits), _dev(c["pre"], bits)
    sd = torch.from_numpy(slabs.copy()).to(DEV)
    xd = _dev(x, bits)
    obuf, out = _padded(tokens, dim, bits)
    rbuf, res = _padded(tokens, dim, bits, _dev(c["res"], bits))
    kernels.gemma_sandwich_norm(out, xd, post, res, pre, G.GEMMA_EPS)
    obuf2, out2 = _padded(tokens, dim, bits)
    rbuf2, res2 = _padded(tokens, dim, bits, _dev(c["res"], bits))
    never = torch.full((tokens, dim), G.CANARY, device=DEV, dtype=torch.int16).view(TDT[bits])   # x is not read
    kernels.gemma_sandwich_norm(out2, never, post, res2, pre, G.GEMMA_EPS,
                                partials=kernels.DeferredPartials.from_slabs(sd))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out2), _bits(out)) and np.array_equal(_bits(res2), _bits(res))
    assert _tail_intact(obuf, rbuf, obuf2, rbuf2) and (_bits(never) == G.CANARY).all()
    # and the x form on that sum meets the caps as every other input does
    _, _, y_ref = G.form_b_ref(x, c["post"], c["res"], c["pre"], bits=bits)
    G.check_residual_b(_bits(res), y_ref, c["res"], f"B slabs residual {bits} {dim}", bits=bits)
    G.check_out(_bits(out), _bits(res), c["pre"], f"B slabs out {bits} {dim}", bits=bits)


@pytest.mark.parametrize("dim,tokens", G.CASES)
@pytest.mark.parametrize("bits", G.BITS)
def test_form_c_embed(bits, dim, tokens):
    from scalellm_amd import kernels
    table, ids, scale, pre, _, want_r = G.embed_case(bits, dim, tokens)
    td, idd, wd = _dev(table, bits), torch.from_numpy(ids.copy()).to(DEV), _dev(pre, bits)
    obuf, out = _padded(tokens, dim, bits)
    rbuf, res = _padded(tokens, dim, bits)
    # handed the unrounded sqrt(hidden): the wrapper rounds it to T, as the reference's T(sqrt(hidden)) is
    kernels.gemma_embed_norm(out, res, td, idd, float(np.sqrt(dim)), wd, G.GEMMA_EPS)
    torch.cuda.synchronize()
    assert scale == G.embed_scale(dim, bits)
    assert np.array_equal(_bits(res), want_r)                      # bit-exact: the gathered row, scaled, one rounding
    share, dist = G.check_out(_bits(out), want_r, pre, f"C {bits} {dim}", bits=bits)
    print(f"\n[gemma-gpu] C {bits} dim {dim}: out share {share:.5f} distance {dist}")
    assert _tail_intact(obuf, rbuf) and np.array_equal(_bits(td), G.f64_to_t_bits(table, bits))
    # x_scale = 1: the gathered row itself
    kernels.gemma_embed_norm(out, res, td, idd, 1.0, wd, G.GEMMA_EPS)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(res), G.f64_to_t_bits(table[ids], bits))


@pytest.mark.parametrize("cap", G.SOFT_CAPS)
@pytest.mark.parametrize("bits", G.BITS)
def test_soft_cap(bits, cap):
    from scalellm_amd import kernels
    x, want, n_planted = G.soft_cap_case(bits, cap)
    rows, row_len = G.SOFT_CAP_SHAPE
    xd = _dev(x, bits)
    obuf, out = _padded(rows, row_len, bits)
    kernels.soft_cap(xd, cap, out=out)
    torch.cuda.synchronize()
    got = _bits(out)
    d = G.t_ulp_distance(got, want)
    share, dist = float((d != 0).mean()), int(d.max())
    print(f"\n[gemma-gpu] soft_cap {bits} cap {cap}: share {share:.5f} distance {dist}; planted worst "
          f"{int(d[0, :n_planted].max())}")
    assert dist <= G.SOFT_CAP_CAP[1] and share <= G.SOFT_CAP_CAP[0], (share, dist)
    assert np.abs(G.t_bits_to_f64(got, bits)).max() <= cap and not torch.isnan(out.float()).any()
    assert _tail_intact(obuf) and np.array_equal(_bits(xd), G.f64_to_t_bits(x, bits))
    kernels.soft_cap(xd, cap)                                      # in place
    torch.cuda.synchronize()
    assert np.array_equal(_bits(xd), got)


@pytest.mark.parametrize("bits", G.BITS)
def test_through_the_pybind_shim(bits):
    """the C++ operator surface gives the bits kernels.* gives: form A (kernel::gemma_rms_norm and the GemmaRMSNorm
    layer), form B, soft_cap"""
    from scalellm_amd import kernels, layers
    shim = _shim()
    dim, tokens = G.CASES[2]
    c = G.norm_case(bits, dim, tokens)
    xd, post, pre = _dev(c["x"], bits), _dev(c["post"], bits), _dev(c["pre"], bits)
    want = torch.empty_like(xd)
    kernels.gemma_rms_norm(want, xd, pre, G.GEMMA_EPS)
    out = torch.empty_like(xd)
    shim.gemma_rms_norm(out, xd, pre, G.GEMMA_EPS)
    layer = shim.GemmaRMSNorm(dim, G.GEMMA_EPS, xd)
    with pytest.raises(RuntimeError):
        layer.verify_loaded_weights("model.norm.")
    layer.load_weight(pre)
    layer.verify_loaded_weights()
    py_layer = layers.GemmaRMSNorm(dim, G.GEMMA_EPS, dtype=TDT[bits], device=DEV)
    with pytest.raises(RuntimeError):
        py_layer.verify_loaded_weights()
    py_layer.load_state_dict({"weight": pre})
    py_layer.verify_loaded_weights()
    with pytest.raises(ValueError):
        py_layer.load_state_dict({"weight": pre[:8]})
    torch.cuda.synchronize()
    for got in (out, layer.forward(xd), py_layer(xd)):
        assert np.array_equal(_bits(got), _bits(want))
    G.check_out(_bits(out), G.f64_to_t_bits(c["x"], bits), c["pre"], f"shim A {bits}", bits=bits)

    res_want, res = _dev(c["res"], bits), _dev(c["res"], bits)
    kernels.gemma_sandwich_norm(want, xd, post, res_want, pre, G.GEMMA_EPS)
    shim.gemma_sandwich_norm(out, xd, post, res, pre, G.GEMMA_EPS)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(_bits(res), _bits(res_want))
    G.check_residual_b(_bits(res), c["y_b"], c["res"], f"shim B {bits}", bits=bits)
    res2 = _dev(c["res"], bits)
    shim.gemma_sandwich_norm(None, xd, post, res2, None, G.GEMMA_EPS)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(res2), _bits(res))

    x, ref_bits, _ = G.soft_cap_case(bits, 30.0)
    ld = _dev(x, bits)
    capped = torch.empty_like(ld)
    shim.soft_cap(capped, ld, 30.0)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(capped), _bits(kernels.soft_cap(ld, 30.0, out=torch.empty_like(ld))))


def test_captured_graph_replays_over_inputs_changed_in_place():
    """forms C -> B -> soft_cap captured once on static buffers; the ids, x and residual are then overwritten in
    place and the replay gives what eager calls give on the new inputs"""
    from scalellm_amd import kernels
    bits, (dim, tokens) = "bf16", G.CASES[2]
    c = G.norm_case(bits, dim, tokens)
    table, ids, scale, pre_c, _, _ = G.embed_case(bits, dim, tokens)
    td, post, pre, pre_cd = _dev(table, bits), _dev(c["post"], bits), _dev(c["pre"], bits), _dev(pre_c, bits)
    idd = torch.zeros(tokens, dtype=torch.int32, device=DEV)
    xd = torch.zeros(tokens, dim, device=DEV, dtype=TDT[bits])
    res, out0, out = torch.empty_like(xd), torch.empty_like(xd), torch.empty_like(xd)

    def step():
        kernels.gemma_embed_norm(out0, res, td, idd, scale, pre_cd, G.GEMMA_EPS)
        kernels.gemma_sandwich_norm(out, xd, post, res, pre, G.GEMMA_EPS)
        kernels.soft_cap(out, 30.0)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    idd.copy_(torch.from_numpy(ids.copy()).to(DEV))                # the inputs change in place after the capture
    xd.copy_(_dev(c["x"], bits))
    graph.replay()
    torch.cuda.synchronize()
    got = [_bits(t).copy() for t in (out0, res, out)]
    step()                                                         # eager, on the same inputs
    torch.cuda.synchronize()
    for g, t in zip(got, (out0, res, out)):
        assert np.array_equal(g, _bits(t))
    want_r0 = G.form_c_ref(table, ids, scale, pre_c, bits=bits)[1]
    _, _, y_ref = G.form_b_ref(c["x"], c["post"], G.t_bits_to_f64(want_r0, bits), c["pre"], bits=bits)
    G.check_residual_b(got[1], y_ref, G.t_bits_to_f64(want_r0, bits), "graph residual", bits=bits)
    assert np.abs(G.t_bits_to_f64(got[2], bits)).max() <= 30.0


def test_limits_are_refused_before_any_launch():
    from scalellm_amd import kernels
    dim = G.DIM_MAX + 8
    x = torch.zeros(2, dim, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(dim, device=DEV, dtype=torch.bfloat16)
    out = torch.full((2, dim), G.CANARY, device=DEV, dtype=torch.int16).view(torch.bfloat16)
    with pytest.raises(kernels.SlmError):
        kernels.gemma_rms_norm(out, x, w, G.GEMMA_EPS)
    with pytest.raises(kernels.SlmError):
        kernels.soft_cap(x[:, :12].contiguous(), 30.0)
    with pytest.raises(kernels.SlmError):
        kernels.gemma_sandwich_norm(out, x, w, x.clone(), None, G.GEMMA_EPS)   # out without pre_weight
    torch.cuda.synchronize()
    assert (_bits(out) == G.CANARY).all()
