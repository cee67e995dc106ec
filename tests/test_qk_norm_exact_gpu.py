"""Bit-level tests of the QK-norm prologue (csrc/qk_norm.hip, slm_hip.h section 19) over the case table of
tests/qk_norm_ref.py: head_dim 64 / 128 / 256, (heads, kv heads) (1, 1) / (3, 1) / (8, 2) / (16, 8) / (40, 8),
1 / 5 / 33 / 70 tokens, both dtypes, both pairings, 16-bit and fp32 tables, dense tensors and column slices of one
padded [q | k | v] row, negative slot ids.

Every run is compared, as 16-bit patterns,
  * with the composition of the existing entry points the section promises the bits of: kernels.rms_norm on
    contiguous copies of q as [T * H, D] rows and of k as [T * KV, D] rows, then slm_rope_kv_append with the append,
    into caches holding the same canary -- whole caches, so a slot nobody names, and every slot when the id is
    negative, keeps the canary; the padding columns of the fused row keep it too;
  * with the float64 reference, stage by stage within the caps tests/glue_ref.py gives RMSNorm and RoPE (a run over
    all-zero positions shows the normalised values: row 0 of the table is the identity rotation);
  * with itself on a second run.
The slab form is run on exactly representable slabs (bit-equal to the plain form on their sum) and on random slabs
against the float64 reference of T(sum in the reduce kernel's order).  A captured launch is replayed over changed
positions and slots.
"""
import numpy as np
import pytest
import torch

from tests import glue_ref as ref
from tests import qk_norm_ref as qref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}


def _dev(vals, bits):
    u = ref.f64_to_t_bits(vals, bits)
    assert np.array_equal(ref.t_bits_to_f64(u, bits), np.asarray(vals, np.float64)), "not values of T"
    return torch.from_numpy(u.view(np.int16)).to(DEV).view(TDT[bits])


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _canary(shape, bits):
    return torch.full(shape, qref.CANARY, device=DEV, dtype=torch.int16).view(TDT[bits])


def _table(kind, bits, D):
    t = qref.table(kind, bits, D)
    return torch.from_numpy(t.astype(np.float32)).to(DEV) if kind == "f32" else _dev(t, bits)


def _layout(case, q, k, v, bits):
    """device (q, k, v views, whole buffer or None) in the case's layout"""
    if not case.fused:
        return _dev(q, bits), _dev(k, bits), _dev(v, bits), None
    buf = _canary((case.T, qref.n_cols(case) + qref.PAD), bits)
    qd, kd, vd = qref.split_row(case, buf[:, :qref.n_cols(case)])
    for d, x in ((qd, q), (kd, k), (vd, v)):
        d.copy_(_dev(x, bits))
    return qd, kd, vd, buf


def _caches(case, bits):
    shape = (qref.n_slots(case), case.n_kv_heads, case.D)
    return _canary(shape, bits), _canary(shape, bits)


def _composition(case, q, k, v, qw, kw, pos, tab, interleaved, slots, bits):
    """(q, k, key cache, value cache) from rms_norm on contiguous [T * heads, D] copies, then slm_rope_kv_append"""
    from scalellm_amd import kernels
    out = []
    for x, w in ((q, qw), (k, kw)):
        rows = _dev(x.reshape(-1, case.D), bits)
        kernels.rms_norm(rows, rows, w, qref.EPS)
        out.append(rows.view(case.T, -1, case.D))
    kc, vc = _caches(case, bits)
    kernels.apply_rotary_pos_emb(out[0], out[1], pos, tab, case.D, interleaved, value=_dev(v, bits), slot_ids=slots,
                                 key_cache=kc, value_cache=vc)
    torch.cuda.synchronize()
    return out[0], out[1], kc, vc


def _run_plain(case, q, k, v, qw, kw, pos, tab, interleaved, slots, bits):
    from scalellm_amd import kernels
    qd, kd, vd, buf = _layout(case, q, k, v, bits)
    kc, vc = _caches(case, bits)
    kernels.qk_norm_rope_kv_append(qd, kd, vd, qw, kw, qref.EPS, pos, tab, interleaved, slot_ids=slots,
                                   key_cache=kc, value_cache=vc)
    torch.cuda.synchronize()
    if buf is not None:
        assert (_bits(buf[:, -qref.PAD:]) == qref.CANARY).all(), "row padding written"
    return qd, kd, vd, kc, vc


def _check_reference(case, q_bits, k_bits, qn_bits, kn_bits, want_qn, want_kn, pos, tab_f64, interleaved, bits, what):
    """the two stages against the float64 reference: the normalised values (run at position 0) within RMS_CAP,
    the rotated ones within ROPE_CAP of the float64 rotation of those normalised values"""
    rms, rope = ref.Pool(), ref.Pool()
    rms.add(qn_bits, want_qn)
    rms.add(kn_bits, want_kn)
    rope.add(q_bits, qref.rope_of(qn_bits, pos, tab_f64, interleaved, bits=bits))
    rope.add(k_bits, qref.rope_of(kn_bits, pos, tab_f64, interleaved, bits=bits))
    print(f"\n[qk-norm] {what}: rms {rms}; rope {rope}")
    rms.check(ref.RMS_CAP, f"qk norm {what}")
    rope.check(ref.ROPE_CAP, f"rope {what}")


@pytest.mark.parametrize("table", qref.TABLES)
@pytest.mark.parametrize("interleaved", (True, False))
@pytest.mark.parametrize("bits", ref.BITS)
@pytest.mark.parametrize("name", [c.name for c in qref.CASES])
def test_plain_form(name, bits, interleaved, table):
    case = qref.BY_NAME[name]
    q, k, v, qw, kw = qref.inputs(name, bits)
    p, s = qref.index(name)
    pos, slots = torch.from_numpy(p).to(DEV), torch.from_numpy(s).to(DEV)
    tab, qwd, kwd = _table(table, bits, case.D), _dev(qw, bits), _dev(kw, bits)
    qd, kd, vd, kc, vc = _run_plain(case, q, k, v, qwd, kwd, pos, tab, interleaved, slots, bits)

    # (1) the bits of the existing kernels, whole caches included
    q2, k2, kc2, vc2 = _composition(case, q, k, v, qwd, kwd, pos, tab, interleaved, slots, bits)
    assert np.array_equal(_bits(qd), _bits(q2)), "q differs from rms_norm + slm_rope_kv_append"
    assert np.array_equal(_bits(kd), _bits(k2)), "k differs from rms_norm + slm_rope_kv_append"
    assert np.array_equal(_bits(kc), _bits(kc2)) and np.array_equal(_bits(vc), _bits(vc2)), "caches differ"
    used = s[s >= 0]
    untouched = np.setdiff1d(np.arange(qref.n_slots(case)), used)
    assert (_bits(kc)[untouched] == qref.CANARY).all() and (_bits(vc)[untouched] == qref.CANARY).all()
    assert np.array_equal(_bits(vc)[used], ref.f64_to_t_bits(v, bits)[s >= 0]), "v is copied"
    assert np.array_equal(_bits(kc)[used], _bits(kd)[s >= 0]), "k in place and in its slot"
    assert np.array_equal(_bits(vd), ref.f64_to_t_bits(v, bits)), "v is an input"

    # (2) the float64 reference, stage by stage
    zero = torch.zeros_like(pos)
    qn, kn, _, _, _ = _run_plain(case, q, k, v, qwd, kwd, zero, tab, interleaved, slots, bits)
    want_qn, want_kn = qref.expected_norm(name, bits)
    _check_reference(case, _bits(qd), _bits(kd), _bits(qn), _bits(kn), want_qn, want_kn, p,
                     qref.table(table, bits, case.D), interleaved, bits,
                     f"{name} {bits} il {int(interleaved)} table {table}")

    # (3) a second run gives the same bits
    qd3, kd3, _, kc3, vc3 = _run_plain(case, q, k, v, qwd, kwd, pos, tab, interleaved, slots, bits)
    for a, b in ((qd3, qd), (kd3, kd), (kc3, kc), (vc3, vc)):
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("bits", ref.BITS)
def test_negative_or_no_slots_rotate_and_leave_the_caches(bits):
    from scalellm_amd import kernels
    case = qref.BY_NAME["d128-h16-t70"]
    q, k, v, qw, kw = qref.inputs(case.name, bits)
    p, s = qref.index(case.name)
    pos, tab, qwd, kwd = torch.from_numpy(p).to(DEV), _table("T", bits, case.D), _dev(qw, bits), _dev(kw, bits)
    qd, kd, _, _, _ = _run_plain(case, q, k, v, qwd, kwd, pos, tab, False, torch.from_numpy(s).to(DEV), bits)
    none = torch.full((case.T,), -1, device=DEV, dtype=torch.int32)
    qn, kn, _, kc, vc = _run_plain(case, q, k, v, qwd, kwd, pos, tab, False, none, bits)
    assert np.array_equal(_bits(qn), _bits(qd)) and np.array_equal(_bits(kn), _bits(kd))
    assert (_bits(kc) == qref.CANARY).all() and (_bits(vc) == qref.CANARY).all()
    qx, kx, vx, buf = _layout(case, q, k, v, bits)                  # slot_ids = None: no append at all
    kernels.qk_norm_rope_kv_append(qx, kx, vx, qwd, kwd, qref.EPS, pos, tab, False)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(qx), _bits(qd)) and np.array_equal(_bits(kx), _bits(kd))
    assert (_bits(buf[:, -qref.PAD:]) == qref.CANARY).all()


def _run_slabs(case, slabs, qw, kw, pos, tab, interleaved, slots, bits):
    """q, k, v are outputs: the column slices of a canary-filled padded row"""
    from scalellm_amd import kernels
    sd = torch.from_numpy(slabs).to(DEV)
    buf = _canary((case.T, qref.n_cols(case) + qref.PAD), bits)
    qd, kd, vd = qref.split_row(case, buf[:, :qref.n_cols(case)])
    kc, vc = _caches(case, bits)
    kernels.qk_norm_rope_kv_append(qd, kd, vd, qw, kw, qref.EPS, pos, tab, interleaved, slot_ids=slots,
                                   key_cache=kc, value_cache=vc, partials=kernels.DeferredPartials.from_slabs(sd))
    torch.cuda.synchronize()
    assert (_bits(buf[:, -qref.PAD:]) == qref.CANARY).all(), "row padding written"
    return qd, kd, vd, kc, vc


@pytest.mark.parametrize("n_splits", qref.SPLITS)
@pytest.mark.parametrize("interleaved", (True, False))
@pytest.mark.parametrize("bits", ref.BITS)
@pytest.mark.parametrize("name", qref.SLAB_CASES)
def test_slab_form(name, bits, interleaved, n_splits):
    case = qref.BY_NAME[name]
    _, _, _, qw, kw = qref.inputs(name, bits)
    p, s = qref.index(name)
    pos, slots = torch.from_numpy(p).to(DEV), torch.from_numpy(s).to(DEV)
    tab, qwd, kwd = _table("f32", bits, case.D), _dev(qw, bits), _dev(kw, bits)
    # (1) exactly representable slabs: the plain form on their sum, bit for bit
    slabs, total = qref.exact_slabs(name, n_splits)
    outs = _run_slabs(case, slabs, qwd, kwd, pos, tab, interleaved, slots, bits)
    q, k, v = qref.split_row(case, total)
    plain = _run_plain(case, q, k, v, qwd, kwd, pos, tab, interleaved, slots, bits)
    for a, b in zip(outs, plain):                                  # v is written in this form
        assert np.array_equal(_bits(a), _bits(b))
    # (2) random slabs: x = T(sum in the reduce kernel's order), then the float64 reference
    slabs = qref.random_slabs(name, n_splits)
    x = ref.round_to_t(qref.splitk_sum_f32(slabs).astype(np.float64), bits)
    q, k, v = qref.split_row(case, x)
    qs, ks, vs, kc, vc = _run_slabs(case, slabs, qwd, kwd, pos, tab, interleaved, slots, bits)
    assert np.array_equal(_bits(vs), ref.f64_to_t_bits(v, bits)), "v = T(sum): owed exactly"
    assert np.array_equal(_bits(vc)[s[s >= 0]], ref.f64_to_t_bits(v, bits)[s >= 0])
    qn, kn, _, _, _ = _run_slabs(case, slabs, qwd, kwd, torch.zeros_like(pos), tab, interleaved, slots, bits)
    _check_reference(case, _bits(qs), _bits(ks), _bits(qn), _bits(kn), qref.norm_ref(q, qw, qref.EPS, bits=bits),
                     qref.norm_ref(k, kw, qref.EPS, bits=bits), p, qref.table("f32", bits, case.D), interleaved,
                     bits, f"slabs {name} {bits} il {int(interleaved)} x{n_splits}")
    # and the plain form on the reduced row gives the same bits
    plain = _run_plain(case, q, k, v, qwd, kwd, pos, tab, interleaved, slots, bits)
    for a, b in zip((qs, ks, vs, kc, vc), plain):
        assert np.array_equal(_bits(a), _bits(b))


def test_captured_launch_replays_over_changed_positions_and_slots():
    from scalellm_amd import kernels
    bits, case = "bf16", qref.BY_NAME["d128-h16-t70"]
    q, k, v, qw, kw = qref.inputs(case.name, bits)
    p, s = qref.index(case.name)
    tab, qwd, kwd = _table("T", bits, case.D), _dev(qw, bits), _dev(kw, bits)
    p2 = ((p.astype(np.int64) * 7 + 3) % qref.MAX_POS).astype(np.int32)
    s2 = np.where(s >= 0, qref.n_slots(case) - 1 - s, s).astype(np.int32)
    s2[case.T // 2], s2[0] = s2[0], -1                             # another padding row
    assert len(set(s2[s2 >= 0].tolist())) == case.T - 1
    pos, slots = torch.from_numpy(p).to(DEV), torch.from_numpy(s).to(DEV)
    qd, kd, vd, buf = _layout(case, q, k, v, bits)
    buf0 = buf.clone()
    kc, vc = _caches(case, bits)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm-up outside the capture
        kernels.qk_norm_rope_kv_append(qd, kd, vd, qwd, kwd, qref.EPS, pos, tab, True, slot_ids=slots,
                                       key_cache=kc, value_cache=vc)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        kernels.qk_norm_rope_kv_append(qd, kd, vd, qwd, kwd, qref.EPS, pos, tab, True, slot_ids=slots,
                                       key_cache=kc, value_cache=vc)
    for pp, ss in ((p2, s2), (p, s)):
        buf.copy_(buf0)
        kc.copy_(_canary(kc.shape, bits)); vc.copy_(_canary(vc.shape, bits))
        pos.copy_(torch.from_numpy(pp)); slots.copy_(torch.from_numpy(ss))
        g.replay()
        torch.cuda.synchronize()
        qe, ke, _, kce, vce = _run_plain(case, q, k, v, qwd, kwd, torch.from_numpy(pp).to(DEV), tab, True,
                                         torch.from_numpy(ss).to(DEV), bits)
        assert np.array_equal(_bits(qd), _bits(qe)) and np.array_equal(_bits(kd), _bits(ke))
        assert np.array_equal(_bits(kc), _bits(kce)) and np.array_equal(_bits(vc), _bits(vce))
