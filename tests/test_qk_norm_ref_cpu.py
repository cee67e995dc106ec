"""CPU tests of the QK-norm prologue boundary (include/slm_hip.h section 19): the symbols are declared, exported and
bound; argument validation is host code that runs before any launch; and the float64 reference of
tests/qk_norm_ref.py is pinned on HuggingFace's own Qwen3RMSNorm + apply_rotary_pos_emb (fp32, CPU) and checked on
hand-worked values."""
import os
import re

import numpy as np
import pytest
import torch

from scalellm_amd import _lib
from tests import glue_ref as ref
from tests import qk_norm_ref as qref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")
OK, INVALID, UNSUPPORTED, ALIGNMENT = 0, -1, -2, -5
F16, BF16, F32 = _lib.SLM_F16, _lib.SLM_BF16, _lib.SLM_F32
P = 4096     # a host address that stands for every pointer: no call below may reach a kernel
ODD = P + 8  # not 16-byte aligned
ENTRIES = ("slm_qk_norm_rope_kv_append", "slm_qk_norm_rope_kv_append_splitk")


def test_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"SLM_API\s+[\w\s\*]+?\b(slm_\w+)\s*\(", src))
    L = _lib.lib()
    for n in ENTRIES:
        assert n in declared, n
        assert getattr(L, n).argtypes is not None, n


def _args(**kw):
    a = dict(q=P, q_ts=3 * 128, k=P, k_ts=128, v=P, v_ts=128, qw=P, kw=P, eps=1e-6, pos=P, cs=P, cs_f32=0, rot=128,
             il=0, slots=P, kc=P, vc=P, T=4, H=3, KV=1, D=128, dtype=BF16)
    a.update(kw)
    return a


def _tail(a):
    return (a["qw"], a["kw"], a["eps"], a["pos"], a["cs"], a["cs_f32"], a["rot"], a["il"], a["slots"], a["kc"],
            a["vc"], a["T"], a["H"], a["KV"], a["D"], a["dtype"], None)


def _plain(**kw):
    a = _args(**kw)
    return _lib.lib().slm_qk_norm_rope_kv_append(a["q"], a["q_ts"], a["k"], a["k_ts"], a["v"], a["v_ts"], *_tail(a))


def _slab(**kw):
    a = _args(**dict(dict(part=P, splits=2, cs_f32=1, il=1, dtype=F16), **kw))
    return _lib.lib().slm_qk_norm_rope_kv_append_splitk(a["part"], a["splits"], a["q"], a["q_ts"], a["k"], a["k_ts"],
                                                        a["v"], a["v_ts"], *_tail(a))


@pytest.mark.parametrize("call", (_plain, _slab))
def test_validation_precedes_any_launch(call):
    # every call below must fail (or be a no-op) on the host: the pointers are not device memory
    assert call(T=0) == OK                                          # a no-op, whatever the pointers
    assert call(T=0, q=None, qw=None, kc=None) == OK
    for name in ("T", "H", "KV", "D", "rot"):
        assert call(**{name: -1}) == INVALID, name
    assert call(H=0) == INVALID and call(KV=0) == INVALID
    for name in ("q", "k", "v", "qw", "kw", "pos", "cs"):
        assert call(**{name: None}) == INVALID, name
    assert call(kc=None) == INVALID and call(vc=None) == INVALID   # caches are needed with slot ids
    assert call(dtype=F32) == UNSUPPORTED
    for d in (32, 80, 96, 192, 512):
        assert call(D=d, rot=d) == UNSUPPORTED, d
    assert call(rot=64) == UNSUPPORTED and call(D=64, rot=128) == UNSUPPORTED
    for name in ("q", "k", "v", "qw", "kw", "cs", "kc", "vc"):
        assert call(**{name: ODD}) == ALIGNMENT, name
    for name in ("q_ts", "k_ts", "v_ts"):
        assert call(**{name: 132}) == ALIGNMENT, name
    # NULL before unsupported before alignment
    assert call(qw=None, D=96, rot=96, kc=ODD) == INVALID and call(D=96, rot=96, kc=ODD) == UNSUPPORTED


def test_form_specific_validation():
    # no slot ids: no append, the caches may be NULL (past the NULL checks, a misaligned q is what is reported)
    assert _plain(slots=None, kc=None, vc=None, q=ODD) == ALIGNMENT
    assert _slab(slots=None, kc=None, vc=None, q=ODD) == ALIGNMENT
    assert _slab(part=None) == INVALID and _slab(splits=0) == INVALID and _slab(splits=-1) == INVALID
    assert _slab(part=ODD) == ALIGNMENT


# ---- the reference itself -----------------------------------------------------------------------------------------
def test_case_table_reaches_every_path():
    names = [c.name for c in qref.CASES]
    assert len(set(names)) == len(names) and set(qref.SLAB_CASES) <= set(names)
    assert {c.fused for c in qref.CASES} == {True, False}
    # more than one wave of head groups: 48 heads at D 256 are 24 wave tasks of 2
    assert qref.tasks_per_token(qref.BY_NAME["d256-h40-t5"], False, False) == 24
    assert any(c.T * qref.tasks_per_token(c, False) % 4 for c in qref.CASES)   # a ragged last workgroup
    assert any((c.n_heads + c.n_kv_heads) % (512 // c.D) for c in qref.CASES)   # a partly used head task
    for c in qref.CASES:
        pos, slots = qref.index(c.name)
        assert pos.max() == qref.MAX_POS - 1 and (c.T < 2 or pos.min() == 0)
        assert c.T < 4 or pos[1] == pos[2]
        live = slots[slots >= 0]
        assert len(set(live.tolist())) == len(live) and live.max() < qref.n_slots(c)
        assert (c.T < 2) == (len(live) == c.T)                                # one padding row where T >= 2


@pytest.mark.parametrize("interleaved", (True, False))
def test_reference_on_hand_worked_values(interleaved):
    """a head of all 2s with weight 3: rs = 1 / sqrt(4 + eps), T(2 rs) = 1, so every normalised value is 3.  Rotation
    by the integer 'angle' (c, s) = (2, 1) of the pair (3, 3): (3 * 2 - 3 * 1, 3 * 2 + 3 * 1) = (3, 9); table row 2
    is the identity."""
    D = 64
    x = np.full((2, 1, D), 2.0)
    tab = np.zeros((3, D))
    tab[1, :D // 2], tab[1, D // 2:] = 2.0, 1.0
    tab[2, :D // 2] = 1.0
    i0, i1 = (0, 1) if interleaved else (0, D // 2)
    for bits in ref.BITS:
        qb, kb = qref.reference(x, x, np.full(D, 3.0), np.full(D, 3.0), 1e-6, np.array([1, 2]), tab, interleaved,
                                bits=bits)
        for b in (qb, kb):
            f = ref.t_bits_to_f64(b, bits)
            assert f[0, 0, i0] == 3.0 and f[0, 0, i1] == 9.0 and (f[1] == 3.0).all()
            assert sorted(set(f[0, 0].tolist())) == [3.0, 9.0]


def test_slab_helpers():
    for name in qref.SLAB_CASES:
        case = qref.BY_NAME[name]
        for n in qref.SPLITS:
            slabs, total = qref.exact_slabs(name, n)
            assert slabs.shape == (n, case.T, qref.n_cols(case))
            assert np.array_equal(qref.splitk_sum_f32(slabs).astype(np.float64), total)
    case = qref.BY_NAME["d128-h3-t5"]
    row = np.arange(case.T * qref.n_cols(case), dtype=np.float64).reshape(case.T, -1)
    q, k, v = qref.split_row(case, row)
    assert q.shape == (5, 3, 128) and k.shape == v.shape == (5, 1, 128)
    assert k[0, 0, 0] == 3 * 128 and v[0, 0, 0] == 4 * 128 and q[1, 0, 0] == qref.n_cols(case)


# ---- the pin on HuggingFace ---------------------------------------------------------------------------------------
# unit roundoff of T: bf16 keeps 8 significant bits, f16 11
UNIT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
# a result in T's subnormal range is rounded to a multiple of this step: half of it absolutely, not u relatively.  The
# norm's first rounding reaches the output times |w| <= 3, its second once: (3 + 1) / 2 steps; the rotation carries
# those through |c| + |s| <= 2 and adds half a step: within 5 steps either way
SUBNORMAL_STEP = {"bf16": 2.0 ** -133, "f16": 2.0 ** -24}


@pytest.mark.parametrize("bits", ref.BITS)
@pytest.mark.parametrize("name", ("d128-h3-t5", "d64-h40-t33", "d256-h8-t33"))
def test_reference_pinned_on_huggingface_qwen3(name, bits):
    """Qwen3Attention's q_norm / k_norm (Qwen3RMSNorm over head_dim, eps = rms_norm_eps) and apply_rotary_pos_emb
    (pairs (i, i + D / 2), cos / sin of Qwen3RotaryEmbedding), run in fp32 on the same values of T, against the float64
    reference, which rounds where the kernels round.  Bounds from the formats alone, u = unit roundoff of T: the
    norm rounds twice (T(x rs), then T(. w)), so |n_ref - n_hf| <= (2u + u^2) |n_hf| plus fp32's own error (2^-20
    relative, covering rsqrt and the mean); the rotation adds one rounding of its result, |out_ref - out_hf| <=
    u |out_hf| + (2u + u^2 + 2^-20)(|a_hf| + |b_hf|) for the pair (a, b) it came from (|cos|, |sin| <= 1; the last
    term also covers fp32's rounding of HF's two products and their sum).  The tables agree with
    Qwen3RotaryEmbedding's to fp32 accuracy at |angle| <= 40."""
    mq = pytest.importorskip("transformers.models.qwen3.modeling_qwen3")
    from transformers import Qwen3Config
    case = qref.BY_NAME[name]
    D = case.D
    q, k, _, qw, kw = qref.inputs(name, bits)
    pos, _ = qref.index(name)
    tab = qref.table("f32", bits, D)
    cfg = Qwen3Config(hidden_size=D * case.n_heads, num_attention_heads=case.n_heads,
                      num_key_value_heads=case.n_kv_heads, head_dim=D, rms_norm_eps=qref.EPS,
                      max_position_embeddings=qref.MAX_POS, rope_parameters={"rope_type": "default",
                                                                          "rope_theta": 1e6})
    rot = mq.Qwen3RotaryEmbedding(cfg)
    x = torch.zeros(1, case.T, D)
    cos, sin = rot(x, torch.from_numpy(pos.astype(np.int64))[None])
    half = D // 2
    cs_tab = torch.from_numpy(np.concatenate([tab[pos, :half], tab[pos, :half]], 1)).float()
    sn_tab = torch.from_numpy(np.concatenate([tab[pos, half:], tab[pos, half:]], 1)).float()
    assert torch.allclose(cos[0], cs_tab, rtol=0, atol=1e-5) and torch.allclose(sin[0], sn_tab, rtol=0, atol=1e-5)

    qn_m, kn_m = mq.Qwen3RMSNorm(D, eps=qref.EPS), mq.Qwen3RMSNorm(D, eps=qref.EPS)
    with torch.no_grad():
        qn_m.weight.copy_(torch.from_numpy(qw.copy()))
        kn_m.weight.copy_(torch.from_numpy(kw.copy()))
        qn = qn_m(torch.from_numpy(q.copy()).float())                      # [T, H, D]
        kn = kn_m(torch.from_numpy(k.copy()).float())
        # HF's layout [batch, heads, T, D], cos / sin [batch, T, D]
        qr, kr = mq.apply_rotary_pos_emb(qn.transpose(0, 1)[None], kn.transpose(0, 1)[None], cs_tab[None],
                                         sn_tab[None])
    qr, kr = qr[0].transpose(0, 1).double().numpy(), kr[0].transpose(0, 1).double().numpy()
    qn, kn = qn.double().numpy(), kn.double().numpy()
    u, f32, tiny = UNIT[bits], 2.0 ** -20, SUBNORMAL_STEP[bits]
    assert np.abs(qw).max() <= 3.0 and np.abs(kw).max() <= 3.0
    nq_b, nk_b = qref.expected_norm(name, bits)
    out_q, out_k = qref.reference(q, k, qw, kw, qref.EPS, pos, tab, False, bits=bits)
    for n_b, n_hf, o_b, o_hf in ((nq_b, qn, out_q, qr), (nk_b, kn, out_k, kr)):
        n_ref = ref.t_bits_to_f64(n_b, bits)
        assert (np.abs(n_ref - n_hf) <= (2 * u + u * u + f32) * np.abs(n_hf) + 5 * tiny).all()
        partner = np.concatenate([n_hf[..., half:], n_hf[..., :half]], -1)
        bound = u * np.abs(o_hf) + (2 * u + u * u + f32) * (np.abs(n_hf) + np.abs(partner)) + 5 * tiny
        assert (np.abs(ref.t_bits_to_f64(o_b, bits) - o_hf) <= bound).all()
        assert np.abs(o_hf).max() > 1.0                             # the comparison is about something
