"""The references and caps behind tests/test_glue_exact_gpu.py, checked without a GPU.

  * the float64 references of tests/glue_ref.py agree with the project's oracle (loosely: the oracle is fp32 and, for
    RMSNorm, rounds once where the kernel rounds twice),
  * an fp32 restatement of the kernel arithmetic (csrc/common.h: rms_sumsq8 / rms_apply8, silu_mul1; csrc/glue.hip:
    rope_rot) on every case's actual inputs -- fp32 h, the fp32 sum of squares in the kernel's order (a sequential
    chain per thread, then a tree), rsqrt off by -8, 0, +8 fp32 ulps, the sigmoid off by +-6, the rotation as an
    fp32 multiply-add -- mismatches the reference in at most HALF of the cap's share and never by more than the
    cap's distance; the residual output is bit-exact,
  * deliberately wrong variants break the caps at least tenfold: RMSNorm with one rounding (the oracle's formula),
    RoPE with the table row or the pair index off by one or the sign of sin flipped, SiLU*mul with gate and up
    swapped.  So the GPU test fails on a subtly wrong kernel,
  * the integer RoPE expectation equals rope_ref bit for bit (a zero has no sign in integers: -0 counts as +0), in
    both dtypes and for both table types.
"""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import glue_ref as ref

BITS = ref.BITS


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _t(x32, bits):
    assert x32.dtype == np.float32
    return ref.helpers._t_bits(x32, bits)


def _t_val(x32, bits):
    """fp32 values of T(x32)"""
    return ref.helpers._from_t_bits(_t(x32, bits), bits)


def _nudge(x32, ulps):
    """normal fp32 values moved by `ulps` patterns; zeros, subnormals, inf and nan stay"""
    u = x32.view(np.int32)
    ok = np.isfinite(x32) & (np.abs(x32) >= np.float32(2.0 ** -126))
    return np.where(ok, u + ulps, u).astype(np.int32).view(np.float32)


# ---- the units --------------------------------------------------------------------------------------------------
def test_ulp_distance_and_single_rounding():
    bf = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x3F80, 0x3F81, 0x007F, 0x0080], np.uint16)
    d = ref.t_ulp_distance
    assert d(bf[0], bf[1]) == 0 and d(bf[2], bf[3]) == 2 and d(bf[4], bf[5]) == 1
    assert d(bf[6], bf[7]) == 1                                    # largest subnormal to smallest normal
    assert d(np.uint16(0x8002), np.uint16(0x0003)) == 5 and d(bf, bf).max() == 0
    for bits, one, ulp in (("bf16", 0x3F80, 2.0 ** -7), ("f16", 0x3C00, 2.0 ** -10)):
        # 1 + ulp/2 is a tie (-> even, 1.0); a float64 hair above it rounds up.  Through fp32 to nearest it would
        # first fall on the tie and then go down: the double rounding f64_to_t_bits is there to avoid
        x = np.array([1.0 + ulp / 2, 1.0 + ulp / 2 + 2.0 ** -40, 1.0 + 3 * ulp / 2, 1.0 + 3 * ulp / 2 - 2.0 ** -40])
        assert ref.f64_to_t_bits(x, bits).tolist() == [one, one + 1, one + 2, one + 1]
        assert ref.f64_to_t_bits(-x, bits).tolist() == [0x8000 + v for v in (one, one + 1, one + 2, one + 1)]
        every = np.arange(0x7C00 if bits == "f16" else 0x7F80, dtype=np.uint16)       # every finite magnitude
        assert np.array_equal(ref.f64_to_t_bits(ref.t_bits_to_f64(every, bits), bits), every)
        assert np.array_equal(ref.t_ulp_distance(every[1:], every[:-1]), np.ones(every.size - 1))


# ---- RMSNorm ----------------------------------------------------------------------------------------------------
def _sumsq_f32(h):
    """The fp32 sum of squares in rms_norm_kernel's order: thread t of 256 runs ONE sequential fma chain over the
    8 columns of its vectors t, t + 256, ... (rms_sumsq8; a masked vector adds nothing), the 64 lanes of a wave
    are summed pairwise (group_sum<64>), the four waves one after the other.  [rows, 1] fp32.
    (One chain over the whole row is not what any thread does, and at dim 16384 it is off by 35 to 135 fp32 ulps
    on these rows: more than the +-8 ulps of rsqrt this restatement is there to vary.)"""
    rows, dim = h.shape
    nv = ref.rms_nv(dim)
    padded = np.zeros((rows, nv * 256 * 8), np.float32)
    padded[:, :dim] = h
    f = padded.reshape(rows, nv, 256, 8).astype(np.float64)
    ss = np.zeros((rows, 256), np.float32)
    for i in range(nv):
        for j in range(8):
            ss = (f[:, i, :, j] * f[:, i, :, j] + ss.astype(np.float64)).astype(np.float32)     # fma: one rounding
    while ss.shape[1] > 4:
        ss = ss[:, 0::2] + ss[:, 1::2]
    assert ss.dtype == np.float32
    return (((ss[:, 0] + ss[:, 1]) + ss[:, 2]) + ss[:, 3])[:, None]


def _rms_f32(x, w, res, bits, ulps, one_rounding=False):
    """the kernel's arithmetic in fp32: (out bits, residual bits)"""
    h = _f32(x)
    res_bits = None
    if res is not None:
        h = h + _f32(res)
        res_bits = _t(h, bits)
    m = _sumsq_f32(h) / np.float32(h.shape[1]) + np.float32(ref.RMS_EPS)
    assert m.dtype == np.float32
    rs = _nudge((1.0 / np.sqrt(m.astype(np.float64))).astype(np.float32), ulps)
    n = h * rs
    if not one_rounding:
        n = _t_val(n, bits)
    return _t(n * _f32(w)[None, :], bits), res_bits


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("dim,tokens", ref.RMS)
@pytest.mark.parametrize("bits", BITS)
def test_rms_norm_reference_and_cap(bits, dim, tokens, with_res):
    x, w, res, want, want_res = ref.rms_case(bits, dim, tokens, with_res)
    # rows: 64 x, 2^-10 x (eps-dominated), zeros
    h = x if res is None else x + res
    ms = (h * h).mean(axis=1)
    assert ms[0] > 100 and ms[1] < ref.RMS_EPS / 4 and (tokens < 3 or ms[2] == 0.0)
    # the oracle (one rounding, fp32): within one ulp of T
    o = oracle.rms_norm(h.astype(np.float32), w.astype(np.float32), ref.RMS_EPS)
    assert ref.t_ulp_distance(_t(o, bits), want).max() <= 1
    worst = (0.0, 0)
    for ulps in (-8, 0, 8):
        got, got_res = _rms_f32(x, w, res, bits, ulps)
        share, dist = ref.mismatch(got, want)
        worst = max(worst, (share, dist))
        assert share <= ref.RMS_CAP[0] / 2 and dist <= ref.RMS_CAP[1], (ulps, share, dist)
        assert res is None or np.array_equal(got_res, want_res)
    print(f"\n[glue-cpu] rms_norm {bits} dim {dim} res {int(with_res)}: share {worst[0]:.5f} distance {worst[1]}")
    if tokens > 2:
        assert not (want[2] & 0x7FFF).any()                        # the zero row gives zeros
    # the oracle's own order of roundings, T(h rs w): what the loose tolerance could not tell apart
    wrong, _ = _rms_f32(x, w, res, bits, 0, one_rounding=True)
    live = slice(0, 2) if tokens == 3 else slice(None)             # a zero row agrees under any formula
    share = ref.mismatch(wrong[live], want[live])[0]
    assert share >= 10 * ref.RMS_CAP[0], share


# ---- SiLU * mul -------------------------------------------------------------------------------------------------
def _silu_f32(x, bits, ulps, swapped=False):
    x32 = _f32(x)
    d = x32.shape[1] // 2
    g, u = (x32[:, d:], x32[:, :d]) if swapped else (x32[:, :d], x32[:, d:])
    with np.errstate(over="ignore"):
        e = np.exp(-g.astype(np.float64)).astype(np.float32)
        sig = _nudge((1.0 / (np.float32(1.0) + e).astype(np.float64)).astype(np.float32), ulps)
    r = g * sig * u
    assert r.dtype == np.float32
    return _t(r, bits)


@pytest.mark.parametrize("tokens,d", ref.SILU)
@pytest.mark.parametrize("bits", BITS)
def test_silu_mul_reference_and_cap(bits, tokens, d):
    x, want = ref.silu_case(bits, tokens, d)
    sub = slice(0, min(tokens, 16))                                # the oracle on a few rows: fp32 against float64
    f64 = ref.silu_mul_f64(x[sub])
    np.testing.assert_allclose(oracle.silu_mul(x[sub].astype(np.float32)), f64, rtol=1e-5, atol=1e-5)
    assert not np.isnan(f64).any()
    for col, g, u in ref.silu_planted(bits, d):
        assert x[0, col] == g and x[0, d + col] == u
        if g == 0.0:
            assert want[0, col] & 0x7FFF == 0
    worst = (0.0, 0)
    for ulps in (-6, 6):
        share, dist = ref.mismatch(_silu_f32(x, bits, ulps), want)
        worst = max(worst, (share, dist))
        assert share <= ref.SILU_CAP[0] / 2 and dist <= ref.SILU_CAP[1], (ulps, share, dist)
    print(f"\n[glue-cpu] silu_mul {bits} {tokens} x {d}: share {worst[0]:.5f} distance {worst[1]}")
    if d > 8:                                                      # (all of the 8-element case is planted pairs)
        share = ref.mismatch(_silu_f32(x, bits, 0, swapped=True), want)[0]
        assert share >= 10 * ref.SILU_CAP[0], share


@pytest.mark.parametrize("bits", BITS)
def test_silu_mul_deep_negative_gates(bits):
    """gates below -60: the scaled fp32 form of silu_mul1 stays within one step of the reference everywhere; the
    plain form with a subnormal sigmoid dropped, as a bare hardware reciprocal does, is off by hundreds in bf16"""
    x, want = ref.silu_deep_case(bits)
    x32 = _f32(x)
    g, u = x32[:, :64], x32[:, 64:]
    # silu_mul1's form: below -64 the sigmoid times 2^32 (exponent argument - 32, 2^-32 for the 1), scaled back last
    k = np.where(g < -64, np.float32(32), np.float32(0))
    one = np.exp2(-k)
    arg = (-g.astype(np.float64) * np.float64(np.float32(1.4426950408889634)) - k).astype(np.float32)       # fma
    e = np.exp2(arg.astype(np.float64)).astype(np.float32)
    assert np.isfinite(e).all()
    for ulps in (-6, 0, 6):
        sig = _nudge((1.0 / (one + e).astype(np.float64)).astype(np.float32), ulps)
        r = g * sig * u * one
        assert r.dtype == np.float32 and ref.mismatch(_t(r, bits), want)[1] <= ref.SILU_CAP[1]
    with np.errstate(over="ignore"):
        sig = (1.0 / (1.0 + np.exp(-g.astype(np.float64)))).astype(np.float32)
    sig[np.abs(sig) < np.float32(2.0 ** -126)] = 0.0               # flushed
    flushed = ref.mismatch(_t(g * sig * u, bits), want)[1]
    assert flushed > 100 if bits == "bf16" else flushed == 0       # (f16 has no number that small)


# ---- RoPE -------------------------------------------------------------------------------------------------------
def _rope_f32(x, pos, table, rot, interleaved, bits, row_off=0, pair_off=0, sin_sign=1.0):
    """rope_rot in fp32: o0 = fma(a, c, -(b s)), o1 = fma(b, c, a s); the fma's single rounding through float64
    (a c is exact there).  row_off / pair_off / sin_sign: the deliberately wrong variants."""
    x32 = _f32(x).copy()
    t32 = _f32(table)
    half = rot // 2
    r = (np.arange(half) + pair_off) % half
    rows = (np.asarray(pos) + row_off) % t32.shape[0]
    c = t32[rows][:, r][:, None, :]
    s = np.float32(sin_sign) * t32[rows][:, half + r][:, None, :]
    i0 = 2 * np.arange(half) if interleaved else np.arange(half)
    i1 = i0 + 1 if interleaved else i0 + half
    a, b = x32[..., i0].copy(), x32[..., i1].copy()
    bs, as_ = (b * s).astype(np.float64), (a * s).astype(np.float64)
    x32[..., i0] = (a.astype(np.float64) * c - bs).astype(np.float32)
    x32[..., i1] = (b.astype(np.float64) * c + as_).astype(np.float32)
    return _t(x32, bits)


@functools.lru_cache(maxsize=None)
def _rope_pool(bits, name):
    """the fp32 restatement on every (pair layout, table type) of a case: a glue_ref.Pool of q and k together;
    every wrong variant breaks the cap tenfold on every combination"""
    case = ref.ROPE_BY_NAME[name]
    pos, _ = ref.rope_index(name)
    pool = ref.Pool()
    for interleaved in (False, True):
        for table in ref.ROPE_TABLES:
            q, k, v, tab, want_q, want_k = ref.rope_real_case(name, interleaved, table, bits)
            want = np.concatenate([want_q.ravel(), want_k.ravel()])

            def both(**kw):
                return np.concatenate([_rope_f32(a, pos, tab, case.rot, interleaved, bits, **kw).ravel()
                                       for a in (q, k)])

            pool.add(both(), want)
            for wrong in (dict(row_off=1), dict(pair_off=1), dict(sin_sign=-1.0)):
                assert ref.mismatch(both(**wrong), want)[0] >= 10 * ref.ROPE_CAP[0], (wrong, interleaved, table)
            # pass-through dims are the input's bits
            assert np.array_equal(want_q[..., case.rot:], ref.f64_to_t_bits(q[..., case.rot:], bits))
    return pool


@pytest.mark.parametrize("case", ref.ROPE, ids=lambda c: c.name)
@pytest.mark.parametrize("bits", BITS)
def test_rope_reference_and_cap(bits, case):
    pool = _rope_pool(bits, case.name)
    print(f"\n[glue-cpu] rope {bits} {case.name}: {pool}")
    pool.check((ref.ROPE_CAP[0] / 2, ref.ROPE_CAP[1]), f"rope {bits} {case.name}")


@pytest.mark.parametrize("path", ["vector", "scalar"])
@pytest.mark.parametrize("bits", BITS)
def test_rope_reference_and_cap_per_kernel(bits, path):
    """every case of one kernel together: this is where the 120 elements of S2 count towards a share"""
    pool = ref.Pool()
    for c in ref.ROPE:
        if c.path == path:
            pool.merge(_rope_pool(bits, c.name))
    print(f"\n[glue-cpu] rope {bits} {path} kernel: {pool}")
    assert pool.n >= ref.SHARE_MIN_ELEMENTS
    pool.check((ref.ROPE_CAP[0] / 2, ref.ROPE_CAP[1]), f"rope {bits} {path}")


@pytest.mark.parametrize("interleaved", [False, True])
def test_rope_reference_against_the_oracle(interleaved):
    """oracle.rope builds its angles in fp32 from inv_freq: give rope_f64 the table of those same angles"""
    rot, D, T = 32, 64, 9
    rng = np.random.default_rng(rot)
    x = rng.standard_normal((T, 3, D)).astype(np.float32)
    pos = rng.integers(0, ref.ROPE_MAX_POS, size=T).astype(np.int32)
    inv = (1.0 / 10000.0 ** (np.arange(0, rot, 2, dtype=np.float32) / rot)).astype(np.float32)
    ang = (np.arange(ref.ROPE_MAX_POS, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float64)
    tab = np.concatenate([np.cos(ang), np.sin(ang)], axis=1)
    np.testing.assert_allclose(oracle.rope(x, pos, inv, rot, interleaved), ref.rope_f64(x, pos, tab, rot, interleaved),
                               rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("case", ref.ROPE, ids=lambda c: c.name)
def test_exact_rope_expectation_is_the_reference(case, interleaved):
    q, k, v, tab, want_q, want_k = ref.rope_exact_case(case.name, interleaved)
    pos, _ = ref.rope_index(case.name)
    for bits in BITS:
        assert np.array_equal(ref.round_to_t(tab, bits), tab)      # the same table as fp32 and as T
        for x, want in ((q, want_q), (k, want_k)):
            got = ref.rope_ref(x, pos, tab, case.rot, interleaved, bits=bits)
            assert ref.same_values(got, ref.f64_to_t_bits(want.astype(np.float64), bits))
            # and the fp32 restatement is exact on it: no rounding anywhere
            assert ref.same_values(_rope_f32(x, pos, tab, case.rot, interleaved, bits), got)
    # a wrong row, pair or sign is seen in many elements, not in a lucky few
    want = ref.f64_to_t_bits(want_q.astype(np.float64), "bf16")
    for wrong in (dict(row_off=1), dict(pair_off=1), dict(sin_sign=-1.0)):
        bad = _rope_f32(q, pos, tab, case.rot, interleaved, "bf16", **wrong)
        assert (bad[..., :case.rot] != want[..., :case.rot]).mean() > 0.5, wrong


def test_rope_case_table_reaches_every_path():
    """the dispatch of slm_rope_kv_append restated (ref.rope_dispatch), on the layouts the GPU test builds"""
    seen = set()
    for c in ref.ROPE:
        for append in (True, False):
            assert ref.rope_case_dispatch(c, append) == (c.path, c.gy)
            seen.add((c.path, c.gy))
    assert seen == {("vector", 1), ("vector", 2), ("vector", 4), ("scalar", 0)}
    # a misaligned pointer alone sends an otherwise aligned layout to the scalar kernel
    v1 = ref.ROPE_BY_NAME["V1"]
    assert ref.rope_case_dispatch(v1, True, pointers=(0, 4, 0, 0, 0)) == ("scalar", 0)
    # append only (no table): always the scalar kernel
    assert ref.rope_dispatch(4, 2, 64, 32, 256, 128, 128, True, has_table=False) == ("scalar", 0)
