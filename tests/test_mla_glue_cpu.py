"""CPU tests of the MLA prologue boundary (include/slm_hip.h section 18) and of slm_moe_sum_add (section 10): the
symbols are declared, exported and bound; argument validation is host code that runs before any launch; and the
float64 reference of tests/mla_glue_ref.py is checked on hand-worked values and against its own building blocks."""
import re
import os

import numpy as np
import pytest

from scalellm_amd import _lib
from tests import glue_ref as ref
from tests import mla_glue_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")
OK, INVALID, UNSUPPORTED, ALIGNMENT = 0, -1, -2, -5
F16, BF16, F32 = _lib.SLM_F16, _lib.SLM_BF16, _lib.SLM_F32
P = 4096     # a host address that stands for every pointer: no call below may reach a kernel
ODD = P + 8  # not 16-byte aligned


def test_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"SLM_API\s+[\w\s\*]+?\b(slm_\w+)\s*\(", src))
    L = _lib.lib()
    for n in ("slm_mla_rope_append", "slm_mla_rope_append_splitk", "slm_moe_sum_add"):
        assert n in declared, n
        assert getattr(L, n).argtypes is not None, n


def _plain(**kw):
    a = dict(q=P, q_ts=3 * 96, kv_a=P, kva_ts=192, w=P, eps=1e-6, pos=P, cs=P, cs_f32=0, il=1, slots=P, kvc=P, krc=P,
             kvc_ss=128, krc_ss=64, T=4, H=3, nope=32, latent=128, rope=64, dtype=BF16)
    a.update(kw)
    return _lib.lib().slm_mla_rope_append(a["q"], a["q_ts"], a["kv_a"], a["kva_ts"], a["w"], a["eps"], a["pos"],
                                          a["cs"], a["cs_f32"], a["il"], a["slots"], a["kvc"], a["krc"], a["kvc_ss"],
                                          a["krc_ss"], a["T"], a["H"], a["nope"], a["latent"], a["rope"], a["dtype"],
                                          None)


def _slab(**kw):
    a = dict(part=P, splits=2, q=P, q_ts=3 * 96, w=P, eps=1e-6, pos=P, cs=P, cs_f32=1, il=0, slots=P, kvc=P, krc=P,
             kvc_ss=128, krc_ss=64, T=4, H=3, nope=32, latent=128, rope=64, dtype=F16)
    a.update(kw)
    return _lib.lib().slm_mla_rope_append_splitk(a["part"], a["splits"], a["q"], a["q_ts"], a["w"], a["eps"],
                                                 a["pos"], a["cs"], a["cs_f32"], a["il"], a["slots"], a["kvc"],
                                                 a["krc"], a["kvc_ss"], a["krc_ss"], a["T"], a["H"], a["nope"],
                                                 a["latent"], a["rope"], a["dtype"], None)


@pytest.mark.parametrize("call", (_plain, _slab))
def test_validation_precedes_any_launch(call):
    # every call below must fail (or be a no-op) on the host: the pointers are not device memory
    assert call(T=0) == OK                                          # a no-op, whatever the pointers
    assert call(T=0, q=None, w=None, kvc=None) == OK
    assert call(T=-1) == INVALID and call(H=-1) == INVALID and call(nope=-8) == INVALID
    for name in ("w", "pos", "cs", "slots", "kvc", "krc", "q"):
        assert call(**{name: None}) == INVALID, name
    assert call(dtype=F32) == UNSUPPORTED
    for latent in (64, 192, 384, 576, 1024):
        assert call(latent=latent) == UNSUPPORTED, latent
    assert call(rope=32) == UNSUPPORTED and call(rope=128) == UNSUPPORTED
    assert call(nope=36) == UNSUPPORTED and call(nope=4) == UNSUPPORTED
    for name in ("q", "w", "cs", "kvc", "krc"):
        assert call(**{name: ODD}) == ALIGNMENT, name
    for name in ("q_ts", "kvc_ss", "krc_ss"):
        assert call(**{name: 100}) == ALIGNMENT, name
    # the order of section 11: NULL before unsupported before alignment
    assert call(w=None, latent=64, kvc=ODD) == INVALID and call(latent=64, kvc=ODD) == UNSUPPORTED


def test_form_specific_validation():
    assert _plain(kv_a=None) == INVALID and _plain(kv_a=ODD) == ALIGNMENT and _plain(kva_ts=196) == ALIGNMENT
    assert _plain(q=None, H=0, T=0) == OK
    assert _slab(part=None) == INVALID and _slab(splits=0) == INVALID and _slab(part=ODD) == ALIGNMENT
    # q = NULL is fine without heads: past the NULL checks, a misaligned cache is what is reported
    assert _plain(q=None, H=0, kvc=ODD) == ALIGNMENT and _slab(q=None, H=0, kvc=ODD) == ALIGNMENT


def test_moe_sum_add_validation():
    f = _lib.lib().slm_moe_sum_add
    assert f(P, P, P, 0, 2, 64, BF16, None) == OK
    assert f(P, P, P, -1, 2, 64, BF16, None) == INVALID
    assert f(P, P, P, 4, 0, 64, BF16, None) == INVALID
    assert f(P, P, P, 4, 2, 0, BF16, None) == INVALID
    assert f(P, P, P, 4, 2, 64, F32, None) == UNSUPPORTED
    assert f(None, P, P, 4, 2, 64, BF16, None) == INVALID
    assert f(P, None, P, 4, 2, 64, BF16, None) == INVALID
    assert f(P, P, None, 4, 2, 64, BF16, None) == INVALID
    for args in ((ODD, P, P), (P, ODD, P), (P, P, ODD)):
        assert f(*args, 4, 2, 64, F16, None) == ALIGNMENT


# ---- the reference itself -----------------------------------------------------------------------------------------
def test_case_table_reaches_every_path():
    names = [c.name for c in mref.CASES]
    assert len(set(names)) == len(names) and set(mref.SLAB_CASES) <= set(names)
    assert {mref.tasks_per_token(c, False) for c in mref.CASES} == {2, 4}       # 8 .. 136 rotary units
    assert mref.tasks_per_token(mref.BY_NAME["h16-t70"], True) == 8             # + 256 pass-through vectors
    assert any(c.T * mref.tasks_per_token(c, False) % 4 for c in mref.CASES)    # a ragged last workgroup
    for c in mref.CASES:
        pos, slots = mref.index(c.name)
        assert pos.max() == mref.MAX_POS - 1 and (c.T < 2 or pos.min() == 0)
        assert c.T < 4 or pos[1] == pos[2]
        live = slots[slots >= 0]
        assert len(set(live.tolist())) == len(live) and live.max() < mref.n_slots(c)
        assert (c.T < 2) == (len(live) == c.T)                                  # one padding row where T >= 2
    assert {c.fused for c in mref.CASES} == {True, False}


@pytest.mark.parametrize("interleaved", (True, False))
def test_reference_on_hand_worked_values(interleaved):
    """latent of all 2s with weight 3: rs = 1 / sqrt(4 + eps), T(2 rs) = 1, so every output is 3.  Rotation by the
    integer 'angle' (c, s) = (2, 1) of the pair (1, 3): (1 * 2 - 3 * 1, 3 * 2 + 1 * 1) = (-1, 7)."""
    latent, nope = 128, 8
    kv_a = np.concatenate([np.full((2, latent), 2.0), np.zeros((2, 64))], axis=1)
    q = np.zeros((2, 1, nope + 64))
    i0, i1 = (0, 1) if interleaved else (0, 32)
    kv_a[:, latent + i0], kv_a[:, latent + i1] = 1.0, 3.0
    q[:, 0, nope + i0], q[:, 0, nope + i1] = 1.0, 3.0
    q[:, 0, :nope] = 5.0
    tab = np.zeros((3, 64))
    tab[1, :32], tab[1, 32:] = 2.0, 1.0
    tab[2, :32] = 1.0                                               # the identity
    for bits in ref.BITS:
        n, k, qq = mref.reference(q, kv_a, np.full(latent, 3.0), 1e-6, np.array([1, 2]), tab, interleaved, latent,
                                  bits=bits)
        assert (ref.t_bits_to_f64(n, bits) == 3.0).all()
        kf, qf = ref.t_bits_to_f64(k, bits), ref.t_bits_to_f64(qq, bits)
        assert kf[0, i0] == -1.0 and kf[0, i1] == 7.0 and kf[1, i0] == 1.0 and kf[1, i1] == 3.0
        assert qf[0, 0, nope + i0] == -1.0 and qf[0, 0, nope + i1] == 7.0 and (qf[:, 0, :nope] == 5.0).all()
        assert np.count_nonzero(kf[0]) == 2 and np.count_nonzero(qf[0, 0, nope:]) == 2


def test_slab_helpers():
    s = np.array([[1e8], [1.0], [-1e8], [1.0], [0.5]], np.float32)
    # ((0 + (1e8 + 1)) + (-1e8 + 1)) + 0.5 in fp32: both ones are absorbed
    assert mref.splitk_sum_f32(s)[0] == np.float32(0.5)
    assert mref.splitk_sum_f32(s[:1])[0] == np.float32(1e8)
    for name in mref.SLAB_CASES:
        for n in mref.SPLITS:
            slabs, total = mref.exact_slabs(name, n)
            assert slabs.shape == (n, mref.BY_NAME[name].T, mref.n_cols(mref.BY_NAME[name]))
            assert np.array_equal(mref.splitk_sum_f32(slabs).astype(np.float64), total)
    case = mref.BY_NAME["h1-t5"]
    row = np.arange(case.T * mref.n_cols(case), dtype=np.float64).reshape(case.T, -1)
    q, kv_a = mref.split_row(case, row)
    assert q.shape == (5, 1, 96) and kv_a.shape == (5, 192) and kv_a[0, 0] == 96 and q[1, 0, 0] == mref.n_cols(case)
