"""Bit-level tests of the glue kernels (csrc/glue.hip: slm_rms_norm, slm_rope_kv_append, slm_silu_mul) on every
dispatch path, against the float64 references of tests/glue_ref.py.

Most bit-identity tests of the suite take these three kernels as their ground truth; tests/test_glue_gpu.py holds
them to ten half-ulps of T at three shapes each, which cannot tell the kernel's two roundings in RMSNorm from the
oracle's one, never reaches the scalar RoPE kernel, gridDim.y > 1 of the vector one, or the second grid-stride
iteration of SiLU*mul.  Here every result is compared as 16-bit patterns, in ulps of T:
  * RMSNorm: NV = 1, 2, 4, 8 with full, partly and fully masked iterations, scaled / eps-dominated / zero rows; the
    residual output bit for bit; the split-K entry on one slab of fp32(x) gives the same bits; in place; the limit,
  * SiLU*mul: one vector, a ragged row, more vectors than the capped grid holds; saturating gates, and gates from
    -60 to -107, where the sigmoid is an fp32 subnormal and silu(g) u still a bf16 number,
  * RoPE + KV append: both kernels, gridDim.y = 1, 2, 4, both pair layouts, fp32 and 16-bit tables, with and without
    the append, column slices of one qkv buffer, a token whose slot id is negative, first and last table row and
    slot, caches and padding filled with a canary.  Once on integers, where every element is owed exactly (wrong
    row, pair, head or column changes bits), once on real angles within the caps.
Each case asserts the kernel it reaches from the dispatch arithmetic of slm_rope_kv_append restated in
glue_ref.rope_dispatch.  The caps are conditions that tests/test_glue_ref_cpu.py shows an fp32 implementation meets
twice over and a subtly wrong one misses tenfold; what the device actually shows is printed and recorded in
glue_ref.MEASURED.
"""
import functools

import numpy as np
import pytest
import torch

from tests import glue_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
SLM_ERR_UNSUPPORTED = -2             # include/slm_hip.h


def _dev(vals, bits):
    """float64 values of T -> device tensor of T, through the bit patterns"""
    u = ref.f64_to_t_bits(vals, bits)
    assert np.array_equal(ref.t_bits_to_f64(u, bits), np.asarray(vals, np.float64)), "not values of T"
    return torch.from_numpy(u.view(np.int16)).to(DEV).view(TDT[bits])


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _nan(shape, bits):
    return torch.full(shape, float("nan"), device=DEV, dtype=TDT[bits])


def _canary(shape, bits):
    return torch.full(shape, ref.CANARY, device=DEV, dtype=torch.int16).view(TDT[bits])


# ---- RMSNorm ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("dim,tokens", ref.RMS)
@pytest.mark.parametrize("bits", ref.BITS)
def test_rms_norm(bits, dim, tokens, with_res):
    from scalellm_amd import kernels
    x, w, res, want, want_res = ref.rms_case(bits, dim, tokens, with_res)
    xd, wd = _dev(x, bits), _dev(w, bits)
    rd = _dev(res, bits) if with_res else None
    out = _nan((tokens, dim), bits)
    kernels.rms_norm(out, xd, wd, ref.RMS_EPS, rd)
    torch.cuda.synchronize()
    got = _bits(out)
    share, dist = ref.mismatch(got, want)
    print(f"\n[glue-gpu] rms_norm {bits} dim {dim} NV{ref.rms_nv(dim)} res {int(with_res)}: share {share:.5f} distance {dist}")
    if with_res:                                                   # T(x + res): one rounding of an fp32 sum
        assert np.array_equal(_bits(rd), want_res)
    ref.assert_within(got, want, ref.RMS_CAP, f"rms_norm {bits} {dim}")
    assert np.array_equal(_bits(xd), ref.f64_to_t_bits(x, bits))   # the input is left alone
    # the split-K entry on ONE slab holding fp32(x): T(sum) = x, so the same bits
    rd2 = _dev(res, bits) if with_res else None
    out2 = _nan((tokens, dim), bits)
    slabs = xd.float()[None].contiguous()
    kernels.rms_norm(out2, xd, wd, ref.RMS_EPS, rd2, partials=kernels.DeferredPartials.from_slabs(slabs))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out2), got)
    if with_res:
        assert np.array_equal(_bits(rd2), want_res)


@pytest.mark.parametrize("bits", ref.BITS)
def test_rms_norm_in_place(bits):
    from scalellm_amd import kernels
    dim, tokens = ref.RMS_INPLACE
    x, w, _, want, _ = ref.rms_case(bits, dim, tokens, False)
    xd, wd = _dev(x, bits), _dev(w, bits)
    out = _nan((tokens, dim), bits)
    kernels.rms_norm(out, xd, wd, ref.RMS_EPS)
    kernels.rms_norm(xd, xd, wd, ref.RMS_EPS)                      # out is x
    torch.cuda.synchronize()
    assert np.array_equal(_bits(xd), _bits(out))
    ref.assert_within(_bits(xd), want, ref.RMS_CAP, f"rms_norm in place {bits}")


def test_rms_norm_limit():
    """dim = 16384 is a case above; 8 more columns are refused before any launch"""
    from scalellm_amd import _lib, kernels
    dim = ref.RMS_DIM_UNSUPPORTED
    assert dim == ref.RMS_DIM_MAX + 8
    x = torch.zeros(2, dim, device=DEV, dtype=torch.bfloat16)
    w = torch.ones(dim, device=DEV, dtype=torch.bfloat16)
    out = _canary((2, dim), "bf16")
    rc = _lib.lib().slm_rms_norm(out.data_ptr(), x.data_ptr(), w.data_ptr(), None, 2, dim, ref.RMS_EPS,
                                 _lib.SLM_BF16, kernels._stream())
    torch.cuda.synchronize()
    assert rc == SLM_ERR_UNSUPPORTED and (_bits(out) == ref.CANARY).all()
    with pytest.raises(kernels.SlmError):
        kernels.rms_norm(out, x, w, ref.RMS_EPS)


# ---- SiLU * mul -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens,d", ref.SILU)
@pytest.mark.parametrize("bits", ref.BITS)
def test_silu_and_mul(bits, tokens, d):
    from scalellm_amd import kernels
    x, want = ref.silu_case(bits, tokens, d)
    xd = _dev(x, bits)
    out = _nan((tokens, d), bits)
    kernels.silu_and_mul(out, xd)
    torch.cuda.synchronize()
    got = _bits(out)
    share, dist = ref.mismatch(got, want)
    print(f"\n[glue-gpu] silu_mul {bits} {tokens} x {d}: share {share:.5f} distance {dist}")
    planted = ref.silu_planted(bits, d)
    print("[glue-gpu]   planted (gate, up, got, want): " + " ".join(
        "(%g, %g, %04x, %04x)" % (g, u, got[0, c], want[0, c]) for c, g, u in planted))
    assert not torch.isnan(out.float()).any()
    for c, g, u in planted:
        if g == 0.0:                                               # +0 and -0 gates: a zero of either sign
            assert got[0, c] & 0x7FFF == 0, (c, g, hex(got[0, c]))
    ref.assert_within(got, want, ref.SILU_CAP, f"silu_mul {bits} {tokens} x {d}")


@pytest.mark.parametrize("bits", ref.BITS)
def test_silu_and_mul_deep_negative_gates(bits):
    """gates from -60 to -107: the sigmoid is an fp32 subnormal below -87.3, which v_rcp_f32 flushes to zero, and
    its exp2 overflows below -88.7, yet silu(g) u is a normal bf16 number there.  Every element within one step."""
    from scalellm_amd import kernels
    x, want = ref.silu_deep_case(bits)
    out = _nan((1, 64), bits)
    kernels.silu_and_mul(out, _dev(x, bits))
    torch.cuda.synchronize()
    got = _bits(out)
    share, dist = ref.mismatch(got, want)
    print(f"\n[glue-gpu] silu_mul {bits} gates -60 .. -107: share {share:.5f} distance {dist}")
    assert dist <= ref.SILU_CAP[1], (dist, [(float(x[0, c]), hex(got[0, c]), hex(want[0, c]))
                                            for c in np.flatnonzero(ref.t_ulp_distance(got, want)[0] > 1)[:6]])


# ---- RoPE + KV append -------------------------------------------------------------------------------------------
def _rope_run(case, bits, interleaved, table_kind, append, q, k, v, table):
    """One slm_rope_kv_append through kernels.apply_rotary_pos_emb on the case's layout; asserts the kernel it
    reaches and everything that does not depend on the values: v, the untouched cache rows, the padding columns.
    Returns the bits of (q, k, the K cache rows of the tokens that have a slot, those tokens)."""
    from scalellm_amd import kernels
    what = f"{case.name} {bits} inter {int(interleaved)} table {table_kind} append {int(append)}"
    T, nh, nkv, D = case.T, case.nh, case.nkv, case.D
    qd, kd, vd = _dev(q, bits), _dev(k, bits), _dev(v, bits)
    buf, pad = None, ref.rope_pad(case)
    if case.layout != "split":
        N = (nh + 2 * nkv) * D
        buf = _canary((T, N + pad), bits)
        buf[:, :nh * D], buf[:, nh * D:(nh + nkv) * D], buf[:, (nh + nkv) * D:N] = (qd.view(T, -1), kd.view(T, -1),
                                                                                 vd.view(T, -1))
        qd, kd, vd = (buf[:, :nh * D].view(T, nh, D), buf[:, nh * D:(nh + nkv) * D].view(T, nkv, D),
                      buf[:, (nh + nkv) * D:N].view(T, nkv, D))
    pos, slots = ref.rope_index(case.name)
    n_slots = ref.rope_n_slots(case)
    kc, vc = _canary((n_slots, nkv, D), bits), _canary((n_slots, nkv, D), bits)
    tab = torch.from_numpy(table.astype(np.float32)).to(DEV) if table_kind == "f32" else _dev(table, bits)
    assert tuple(tab.shape) == (ref.ROPE_MAX_POS, case.rot) and int(pos.max()) == ref.ROPE_MAX_POS - 1
    # the kernel this call reaches, from the strides and pointers it is given
    strides = (qd.stride(0), kd.stride(0), vd.stride(0) if append else 0)
    assert strides == ref.rope_token_strides(case, append), (what, strides)
    pointers = (qd.data_ptr(), kd.data_ptr()) + ((vd.data_ptr(), kc.data_ptr(), vc.data_ptr()) if append else (0, 0, 0))
    assert ref.rope_case_dispatch(case, append, pointers) == (case.path, case.gy), what
    kernels.apply_rotary_pos_emb(qd, kd, torch.from_numpy(pos.copy()).to(DEV), tab, case.rot, interleaved,
                                 value=vd if append else None,
                                 slot_ids=torch.from_numpy(slots.copy()).to(DEV) if append else None,
                                 key_cache=kc if append else None, value_cache=vc if append else None)
    torch.cuda.synchronize()
    q_bits, k_bits, kc_bits, vc_bits = _bits(qd), _bits(kd), _bits(kc), _bits(vc)
    v_in = ref.f64_to_t_bits(v, bits)
    assert np.array_equal(_bits(vd), v_in), what                   # v is only read
    if buf is not None:                                            # the columns outside q / k / v
        assert (_bits(buf)[:, -pad:] == ref.CANARY).all(), what
    toks = np.flatnonzero(slots >= 0) if append else np.zeros(0, np.int64)
    untouched = np.ones(n_slots, bool)
    untouched[slots[toks]] = False
    assert untouched.sum() == n_slots - (case.T - 1 if append else 0)      # the slot -1 token went nowhere
    assert (kc_bits[untouched] == ref.CANARY).all() and (vc_bits[untouched] == ref.CANARY).all(), what
    # the append is a bit-exact copy of the in-place k and of v
    assert np.array_equal(kc_bits[slots[toks]], k_bits[toks]), what
    assert np.array_equal(vc_bits[slots[toks]], v_in[toks]), what
    return q_bits, k_bits, kc_bits[slots[toks]], toks


def _combos():
    return [(i, t, a) for i in (False, True) for t in ref.ROPE_TABLES for a in (True, False)]


@pytest.mark.parametrize("case", ref.ROPE, ids=lambda c: c.name)
@pytest.mark.parametrize("bits", ref.BITS)
def test_rope_kv_append_exact(bits, case):
    """integers: every element of q, k and the K / V cache rows is owed exactly (-0 counts as +0)"""
    for interleaved, table_kind, append in _combos():
        q, k, v, table, want_q, want_k = ref.rope_exact_case(case.name, interleaved)
        q_bits, k_bits, kc_rows, toks = _rope_run(case, bits, interleaved, table_kind, append, q, k, v, table)
        what = f"{case.name} {bits} inter {int(interleaved)} table {table_kind} append {int(append)}"
        wq, wk = (ref.f64_to_t_bits(w.astype(np.float64), bits) for w in (want_q, want_k))
        for got, want, name in ((q_bits, wq, "q"), (k_bits, wk, "k"), (kc_rows, wk[toks], "key cache")):
            bad = ref.t_ulp_distance(got, want) != 0
            assert not bad.any(), (what, name, "%d elements differ, first (token, head, dim): %s" % (
                bad.sum(), np.argwhere(bad)[:4].tolist()))


@functools.lru_cache(maxsize=None)
def _rope_real_pool(bits, name):
    """real angles, every combination of one case: the distance cap on every run, the mismatches pooled"""
    case = ref.ROPE_BY_NAME[name]
    pool = ref.Pool()
    for interleaved, table_kind, append in _combos():
        q, k, v, table, want_q, want_k = ref.rope_real_case(name, interleaved, table_kind, bits)
        q_bits, k_bits, _, _ = _rope_run(case, bits, interleaved, table_kind, append, q, k, v, table)
        run = ref.Pool()
        run.add(q_bits, want_q)
        run.add(k_bits, want_k)
        assert run.dist <= ref.ROPE_CAP[1], (name, bits, interleaved, table_kind, append, str(run))
        # pass-through dims are copies
        assert np.array_equal(q_bits[..., case.rot:], want_q[..., case.rot:])
        assert np.array_equal(k_bits[..., case.rot:], want_k[..., case.rot:])
        pool.merge(run)
    return pool


@pytest.mark.parametrize("case", ref.ROPE, ids=lambda c: c.name)
@pytest.mark.parametrize("bits", ref.BITS)
def test_rope_kv_append_real_angles(bits, case):
    pool = _rope_real_pool(bits, case.name)
    print(f"\n[glue-gpu] rope {bits} {case.name} ({case.path}, gy {case.gy}): {pool}")
    pool.check(ref.ROPE_CAP, f"rope {bits} {case.name}")


@pytest.mark.parametrize("path", ["vector", "scalar"])
@pytest.mark.parametrize("bits", ref.BITS)
def test_rope_kv_append_real_angles_per_kernel(bits, path):
    """the cases of one kernel together (glue_ref.SHARE_MIN_ELEMENTS: where S2's 120 elements count)"""
    pool = ref.Pool()
    for c in ref.ROPE:
        if c.path == path:
            pool.merge(_rope_real_pool(bits, c.name))
    print(f"\n[glue-gpu] rope {bits} {path} kernel: {pool}")
    assert pool.n >= ref.SHARE_MIN_ELEMENTS
    pool.check(ref.ROPE_CAP, f"rope {bits} {path}")


@pytest.mark.parametrize("name", ["V1", "S2"])
@pytest.mark.parametrize("bits", ref.BITS)
def test_rope_kv_append_without_a_table(bits, name):
    """cos_sin = NULL through the C ABI: append only (alibi models), on an aligned layout and on S2's.  The caches
    receive k and v unrotated; q and k are untouched; the token with slot -1 is skipped."""
    from scalellm_amd import _lib, kernels
    case = ref.ROPE_BY_NAME[name]
    q, k, v, _, _, _ = ref.rope_real_case(name, False, "f32", bits)
    qd, kd, vd = _dev(q, bits), _dev(k, bits), _dev(v, bits)
    _, slots = ref.rope_index(name)
    n_slots = ref.rope_n_slots(case)
    kc, vc = _canary((n_slots, case.nkv, case.D), bits), _canary((n_slots, case.nkv, case.D), bits)
    sd = torch.from_numpy(slots.copy()).to(DEV)
    assert ref.rope_dispatch(case.nh, case.nkv, case.D, case.rot, qd.stride(0), kd.stride(0), vd.stride(0), True,
                             has_table=False) == ("scalar", 0)
    rc = _lib.lib().slm_rope_kv_append(qd.data_ptr(), qd.stride(0), kd.data_ptr(), kd.stride(0), vd.data_ptr(),
                                       vd.stride(0), None, None, 1, case.rot, 0, sd.data_ptr(), kc.data_ptr(),
                                       vc.data_ptr(), case.T, case.nh, case.nkv, case.D, kernels._dtype_code(qd),
                                       kernels._stream())
    torch.cuda.synchronize()
    assert rc == 0
    k_in, v_in = ref.f64_to_t_bits(k, bits), ref.f64_to_t_bits(v, bits)
    assert np.array_equal(_bits(qd), ref.f64_to_t_bits(q, bits)) and np.array_equal(_bits(kd), k_in)
    assert np.array_equal(_bits(vd), v_in)
    toks = np.flatnonzero(slots >= 0)
    assert np.array_equal(_bits(kc)[slots[toks]], k_in[toks]) and np.array_equal(_bits(vc)[slots[toks]], v_in[toks])
    untouched = np.ones(n_slots, bool)
    untouched[slots[toks]] = False
    assert (_bits(kc)[untouched] == ref.CANARY).all() and (_bits(vc)[untouched] == ref.CANARY).all()
