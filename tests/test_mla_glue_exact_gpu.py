"""Bit-level tests of the MLA prologue (csrc/mla_glue.hip, slm_hip.h section 18) over the case table of
tests/mla_glue_ref.py: latent 128 / 256 / 512, nope 32 / 128, 0 / 1 / 3 / 16 heads, 1 / 5 / 33 / 70 tokens, both
dtypes, both pairings, 16-bit and fp32 tables, dense tensors and column slices of one padded row.

Every run is compared, as 16-bit patterns,
  * with the kernels the section promises the bits of: kernels.rms_norm on a contiguous copy of the latent columns,
    slm_rope_kv_append on contiguous copies of the query tails and the key viewed as 64-wide heads, and whole caches
    against kernels.mla_set_kv_cache of those results into caches holding the same canary -- which also shows that a
    slot nobody names, and every slot when the id is negative, keeps the canary;
  * with the float64 reference, within the caps tests/glue_ref.py gives RMSNorm and RoPE;
  * with itself on a second run.
The slab form is run on exactly representable slabs (any order of addition is exact: bit-equal to the plain form on
their sum) and on random slabs against the float64 reference of T(sum in the reduce kernel's order).  A captured
launch is replayed over changed positions and slots.
"""
import numpy as np
import pytest
import torch

from tests import glue_ref as ref
from tests import mla_glue_ref as mref

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
    return torch.full(shape, mref.CANARY, device=DEV, dtype=torch.int16).view(TDT[bits])


def _table(kind, bits):
    t = mref.table(kind, bits)
    return torch.from_numpy(t.astype(np.float32)).to(DEV) if kind == "f32" else _dev(t, bits)


def _layout(case, q, kv_a, bits):
    """device (q view or None, kv_a view, whole buffer or None) in the case's layout"""
    if not case.fused:
        return (_dev(q, bits) if q is not None else None), _dev(kv_a, bits), None
    qc = case.n_heads * (case.nope + mref.ROPE)
    buf = _canary((case.T, mref.n_cols(case) + 8), bits)
    kd = buf[:, qc:qc + case.latent + mref.ROPE]
    kd.copy_(_dev(kv_a, bits))
    qd = None
    if q is not None:
        qd = buf[:, :qc].view(case.T, case.n_heads, case.nope + mref.ROPE)
        qd.copy_(_dev(q, bits))
    return qd, kd, buf


def _caches(case, bits):
    return _canary((mref.n_slots(case), case.latent), bits), _canary((mref.n_slots(case), mref.ROPE), bits)


def _existing_kernels(case, q, kv_a, w, pos, tab, interleaved, slots, bits):
    """(kv cache, rope-key cache, rotated heads [T, H + 1, 64]) from rms_norm, slm_rope_kv_append and
    mla_set_kv_cache on contiguous copies"""
    from scalellm_amd import kernels
    c = _dev(kv_a[:, :case.latent], bits)
    n = torch.empty_like(c)
    kernels.rms_norm(n, c, w, mref.EPS)
    tails = [kv_a[:, None, case.latent:]] if q is None else [q[:, :, case.nope:], kv_a[:, None, case.latent:]]
    heads = _dev(np.concatenate(tails, axis=1), bits)              # query tails, then the key: 64-wide heads
    dummy = torch.zeros(case.T, 1, mref.ROPE, device=DEV, dtype=TDT[bits])
    kernels.apply_rotary_pos_emb(heads, dummy, pos, tab, mref.ROPE, interleaved)
    kvc, krc = _caches(case, bits)
    kernels.mla_set_kv_cache(slots, n, heads[:, -1].contiguous(), kvc, krc)
    return kvc, krc, heads


def _run_plain(case, q, kv_a, w, pos, tab, interleaved, slots, bits):
    from scalellm_amd import kernels
    qd, kd, buf = _layout(case, q, kv_a, bits)
    kvc, krc = _caches(case, bits)
    kernels.mla_rope_append(qd, kd, w, mref.EPS, pos, tab, interleaved, slots, kvc, krc, case.nope)
    torch.cuda.synchronize()
    return qd, kd, buf, kvc, krc


@pytest.mark.parametrize("table", ("T", "f32"))
@pytest.mark.parametrize("interleaved", (True, False))
@pytest.mark.parametrize("bits", ref.BITS)
@pytest.mark.parametrize("name", [c.name for c in mref.CASES])
def test_plain_form(name, bits, interleaved, table):
    case = mref.BY_NAME[name]
    q, kv_a, w = mref.inputs(name, bits)
    p, s = mref.index(name)
    pos, slots = torch.from_numpy(p).to(DEV), torch.from_numpy(s).to(DEV)
    tab, wd = _table(table, bits), _dev(w, bits)
    qd, kd, buf, kvc, krc = _run_plain(case, q, kv_a, wd, pos, tab, interleaved, slots, bits)

    # (1) the bits of the existing kernels, whole caches included
    kvc2, krc2, heads = _existing_kernels(case, q, kv_a, wd, pos, tab, interleaved, slots, bits)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(kvc), _bits(kvc2)), "latent rows differ from rms_norm + mla_set_kv_cache"
    assert np.array_equal(_bits(krc), _bits(krc2)), "rotated keys differ from slm_rope_kv_append + mla_set_kv_cache"
    used = s[s >= 0]
    untouched = np.setdiff1d(np.arange(mref.n_slots(case)), used)
    assert (_bits(kvc)[untouched] == mref.CANARY).all() and (_bits(krc)[untouched] == mref.CANARY).all()
    assert not (_bits(kvc)[used] == mref.CANARY).all(axis=1).any()
    if q is not None:
        assert np.array_equal(_bits(qd[:, :, case.nope:]), _bits(heads[:, :-1])), "query tails differ"
        assert np.array_equal(_bits(qd[:, :, :case.nope]), ref.f64_to_t_bits(q[:, :, :case.nope], bits)), "nope written"
    assert np.array_equal(_bits(kd), ref.f64_to_t_bits(kv_a, bits)), "kv_a is an input"
    if buf is not None:
        assert (_bits(buf[:, -8:]) == mref.CANARY).all(), "row padding written"

    # (2) the float64 reference
    n_ref, k_ref, q_ref = mref.expected(name, bits, interleaved, table)
    rms, rope = ref.Pool(), ref.Pool()
    rms.add(_bits(kvc)[used], n_ref[s >= 0])
    rope.add(_bits(krc)[used], k_ref[s >= 0])
    if q is not None:
        rope.add(_bits(qd), q_ref)
    print(f"\n[mla-glue] {name} {bits} il {int(interleaved)} table {table}: rms {rms}; rope {rope}")
    rms.check(ref.RMS_CAP, f"latent norm {name}")
    rope.check(ref.ROPE_CAP, f"rope {name}")

    # (3) a second run gives the same bits
    qd3, _, _, kvc3, krc3 = _run_plain(case, q, kv_a, wd, pos, tab, interleaved, slots, bits)
    assert np.array_equal(_bits(kvc3), _bits(kvc)) and np.array_equal(_bits(krc3), _bits(krc))
    if q is not None:
        assert np.array_equal(_bits(qd3), _bits(qd))


@pytest.mark.parametrize("bits", ref.BITS)
def test_negative_slots_rotate_q_and_leave_the_caches(bits):
    case = mref.BY_NAME["h3-t5"]
    q, kv_a, w = mref.inputs(case.name, bits)
    p, s = mref.index(case.name)
    pos, tab, wd = torch.from_numpy(p).to(DEV), _table("T", bits), _dev(w, bits)
    qd, _, _, _, _ = _run_plain(case, q, kv_a, wd, pos, tab, True, torch.from_numpy(s).to(DEV), bits)
    none = torch.full((case.T,), -1, device=DEV, dtype=torch.int32)
    qn, _, _, kvc, krc = _run_plain(case, q, kv_a, wd, pos, tab, True, none, bits)
    assert np.array_equal(_bits(qn), _bits(qd))
    assert (_bits(kvc) == mref.CANARY).all() and (_bits(krc) == mref.CANARY).all()


def _run_slabs(case, slabs, w, pos, tab, interleaved, slots, bits):
    from scalellm_amd import kernels
    sd = torch.from_numpy(slabs).to(DEV)
    qc = case.n_heads * (case.nope + mref.ROPE)
    buf = _canary((case.T, qc + 8), bits)                          # q is an output with a padded row
    qd = buf[:, :qc].view(case.T, case.n_heads, case.nope + mref.ROPE) if case.n_heads else None
    kvc, krc = _caches(case, bits)
    kernels.mla_rope_append(qd, None, w, mref.EPS, pos, tab, interleaved, slots, kvc, krc, case.nope,
                            partials=kernels.DeferredPartials.from_slabs(sd))
    torch.cuda.synchronize()
    assert (_bits(buf[:, qc:]) == mref.CANARY).all()
    return qd, kvc, krc


@pytest.mark.parametrize("n_splits", mref.SPLITS)
@pytest.mark.parametrize("interleaved", (True, False))
@pytest.mark.parametrize("bits", ref.BITS)
@pytest.mark.parametrize("name", mref.SLAB_CASES)
def test_slab_form(name, bits, interleaved, n_splits):
    case = mref.BY_NAME[name]
    _, _, w = mref.inputs(name, bits)
    p, s = mref.index(name)
    pos, slots = torch.from_numpy(p).to(DEV), torch.from_numpy(s).to(DEV)
    tab, wd = _table("f32", bits), _dev(w, bits)
    # (1) exactly representable slabs: the plain form on their sum, bit for bit
    slabs, total = mref.exact_slabs(name, n_splits)
    qs, kvc, krc = _run_slabs(case, slabs, wd, pos, tab, interleaved, slots, bits)
    q, kv_a = mref.split_row(case, total)
    qp, _, _, kvc2, krc2 = _run_plain(case, q, kv_a, wd, pos, tab, interleaved, slots, bits)
    assert np.array_equal(_bits(kvc), _bits(kvc2)) and np.array_equal(_bits(krc), _bits(krc2))
    if q is not None:
        assert np.array_equal(_bits(qs), _bits(qp))               # the nope columns are written in this form
    # (2) random slabs: x = T(sum in the reduce kernel's order), then the float64 reference
    slabs = mref.random_slabs(name, n_splits)
    x = ref.round_to_t(mref.splitk_sum_f32(slabs).astype(np.float64), bits)
    q, kv_a = mref.split_row(case, x)
    n_ref, k_ref, q_ref = mref.reference(q, kv_a, w, mref.EPS, p, mref.table("f32", bits), interleaved, case.latent,
                                         bits=bits)
    qs, kvc, krc = _run_slabs(case, slabs, wd, pos, tab, interleaved, slots, bits)
    used = s[s >= 0]
    rms, rope = ref.Pool(), ref.Pool()
    rms.add(_bits(kvc)[used], n_ref[s >= 0])
    rope.add(_bits(krc)[used], k_ref[s >= 0])
    if q is not None:
        rope.add(_bits(qs), q_ref)
        assert np.array_equal(_bits(qs[:, :, :case.nope]), q_ref[:, :, :case.nope])   # T(sum): owed exactly
    print(f"\n[mla-glue] slabs {name} {bits} il {int(interleaved)} x{n_splits}: rms {rms}; rope {rope}")
    rms.check(ref.RMS_CAP, f"latent norm {name}")
    rope.check(ref.ROPE_CAP, f"rope {name}")
    # and the plain form on the reduced row gives the same bits
    qp, _, _, kvc2, krc2 = _run_plain(case, q, kv_a, wd, pos, tab, interleaved, slots, bits)
    assert np.array_equal(_bits(kvc), _bits(kvc2)) and np.array_equal(_bits(krc), _bits(krc2))
    if q is not None:
        assert np.array_equal(_bits(qs), _bits(qp))


def test_captured_launch_replays_over_changed_positions_and_slots():
    from scalellm_amd import kernels
    bits, case = "bf16", mref.BY_NAME["h16-t70"]
    q, kv_a, w = mref.inputs(case.name, bits)
    p, s = mref.index(case.name)
    tab, wd = _table("T", bits), _dev(w, bits)
    p2 = ((p.astype(np.int64) * 7 + 3) % mref.MAX_POS).astype(np.int32)
    s2 = np.where(s >= 0, mref.n_slots(case) - 1 - s, s).astype(np.int32)
    s2[case.T // 2], s2[0] = s2[0], -1                             # another padding row
    assert len(set(s2[s2 >= 0].tolist())) == case.T - 1
    pos, slots = torch.from_numpy(p).to(DEV), torch.from_numpy(s).to(DEV)
    qd, kd, _ = _layout(case, q, kv_a, bits)
    q0 = qd.clone()
    kvc, krc = _caches(case, bits)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm-up outside the capture
        kernels.mla_rope_append(qd, kd, wd, mref.EPS, pos, tab, True, slots, kvc, krc, case.nope)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        kernels.mla_rope_append(qd, kd, wd, mref.EPS, pos, tab, True, slots, kvc, krc, case.nope)
    for pp, ss in ((p2, s2), (p, s)):
        qd.copy_(q0)
        kvc.copy_(_canary(kvc.shape, bits)); krc.copy_(_canary(krc.shape, bits))
        pos.copy_(torch.from_numpy(pp)); slots.copy_(torch.from_numpy(ss))
        g.replay()
        torch.cuda.synchronize()
        qe, _, _, kvce, krce = _run_plain(case, q, kv_a, wd, torch.from_numpy(pp).to(DEV), tab, True,
                                          torch.from_numpy(ss).to(DEV), bits)
        assert np.array_equal(_bits(qd), _bits(qe))
        assert np.array_equal(_bits(kvc), _bits(kvce)) and np.array_equal(_bits(krc), _bits(krce))
