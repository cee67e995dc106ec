"""Float64 references and case tables of the glue-kernel bit tests: what tests/test_glue_exact_gpu.py runs on the
device (slm_rms_norm, slm_rope_kv_append, slm_silu_mul: csrc/glue.hip) and what tests/test_glue_ref_cpu.py checks
the references and the caps on without one.  Imports no GPU code.

A result is compared as 16-bit patterns of T, in ulps of T (t_ulp_distance), against the kernel's OWN order of
roundings evaluated in float64: RMSNorm T(T(h rs) w) on the fp32 h = x + residual (rms_apply8, csrc/common.h),
SiLU*mul T(g / (1 + exp(-g)) u) (silu_mul1), RoPE T(a c - b s), T(b c + a s) (rope_rot).  The kernels evaluate
the same expressions in fp32 with the hardware's rsq / exp / rcp (1 ulp of fp32 each), so they may land on the
other side of a rounding boundary of T in a small share of elements, by one step.  The caps below bound that share;
they are conditions, not measurements: tests/test_glue_ref_cpu.py shows that an fp32 restatement of the kernel
arithmetic with its rsqrt off by +-8 fp32 ulps, its sigmoid by +-6, stays below HALF of each share and inside each
distance, and that a kernel with another order of roundings (the oracle's single rounding in RMSNorm), a table row
or pair index off by one, the sign of sin flipped or gate and up swapped exceeds them at least tenfold.

              cap: share, distance | fp32 restatement on the CPU, worst case | MI355X, worst case (MEASURED)
  RMSNorm  bf16    0.5 %   2 ulps   |  0.046 %  2                              |  0.015 %  2
           f16                      |  0.168 %  2                              |  0.016 %  2
  SiLU*mul bf16    0.5 %   1 ulp    |  0.017 %  1                              |  0.002 %  1
           f16                      |  0.070 %  1                              |  0.010 %  1
  RoPE     bf16    0.1 %   1 ulp    |  0.002 %  1  (one case, tables pooled)   |  0.002 %  1
           f16                      |  0.026 %  1                              |  0.026 %  1
The device stays far below the restatement in RMSNorm because its rsqrt is within one fp32 ulp, not eight.

One finding came out of the planted SiLU gates: at g = -88 the kernel returned 0 where bf16 owes -88 sigmoid(-88) u
= 4.0e-37 (pattern 0308, a NORMAL bf16 number, 776 steps from zero): sigmoid(-88) = 6.1e-39 is an fp32 subnormal and
v_rcp_f32 flushes a subnormal result to zero.  No cap was widened for it; silu_mul1 (csrc/common.h) now carries the
sigmoid times 2^32 below g = -64 (silu_deep_case below walks the gates from -60 to -107).
"""
import functools
from collections import namedtuple

import numpy as np

from tests import helpers

BITS = ("bf16", "f16")
CANARY = 0x7B7B                       # a finite, unlikely value in both formats: caches and padding columns hold it

# cap on the share of a case's elements that differ from the reference, and on the distance of any element
RMS_CAP = (0.005, 2)
SILU_CAP = (0.005, 1)
ROPE_CAP = (0.001, 1)

# share of mismatching elements and largest distance seen on an MI355X (gfx950), worst case per kernel and dtype
MEASURED = {
    ("rms_norm", "bf16"): (0.00015, 2), ("rms_norm", "f16"): (0.00016, 2),
    ("silu_mul", "bf16"): (0.00002, 1), ("silu_mul", "f16"): (0.00010, 1),
    ("rope", "bf16"): (0.00002, 1), ("rope", "f16"): (0.00026, 1),
}


# ---- T <-> float64 ----------------------------------------------------------------------------------------------
def f64_to_t_bits(x, bits):
    """RNE_T of float64 values as uint16 patterns, rounded ONCE: float64 -> fp32 by round-to-odd (the sticky bit
    survives), then fp32 -> T to nearest even, which is exact because T keeps at least 13 bits fewer than fp32."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        r = x.astype(np.float32)
    u = r.view(np.uint32).copy()
    inexact = np.isfinite(r) & (r.astype(np.float64) != x) & ((u & 1) == 0)
    # r was rounded to an even pattern: the odd neighbour on x's side is the round-to-odd result
    away = np.abs(r.astype(np.float64)) < np.abs(x)
    u = np.where(inexact & away, u + 1, np.where(inexact & ~away, u - 1, u)).astype(np.uint32)
    return helpers._t_bits(u.view(np.float32).reshape(x.shape), bits)


def t_bits_to_f64(u16, bits):
    return helpers._from_t_bits(np.ascontiguousarray(u16, dtype=np.uint16), bits).astype(np.float64)


def round_to_t(x, bits):
    """float64 values of RNE_T(x)"""
    return t_bits_to_f64(f64_to_t_bits(x, bits), bits)


def t_ulp_distance(got_bits, ref_bits):
    """Distance in units of T between 16-bit patterns (bf16 or f16: both sign-magnitude, so the pattern below the
    sign bit orders the magnitudes, subnormals included; -0 and +0 are 0 apart)."""
    def ordered(u):
        u = np.asarray(u).astype(np.uint16).astype(np.int32)
        mag = u & 0x7FFF
        return np.where(u & 0x8000, -mag, mag)
    return np.abs(ordered(got_bits) - ordered(ref_bits))


def mismatch(got_bits, ref_bits):
    """(share of elements that differ, largest distance)"""
    d = t_ulp_distance(got_bits, ref_bits)
    return float((d != 0).mean()), int(d.max())


def same_values(got_bits, ref_bits):
    """bit equality, except that -0 is +0: (-3) * 0 is -0 in floating point and 0 in integers"""
    return got_bits.shape == ref_bits.shape and not t_ulp_distance(got_bits, ref_bits).any()


def assert_within(got_bits, ref_bits, cap, what):
    share, dist = mismatch(got_bits, ref_bits)
    assert share <= cap[0] and dist <= cap[1], (what, "share %.5f of cap %.5f" % (share, cap[0]),
                                                "distance %d of cap %d" % (dist, cap[1]))
    return share, dist


# A share cap means something only over enough elements: below 1 / cap of them it allows no mismatch at all, which
# is bit equality, and an fp32 kernel does not owe that against a float64 reference.  Every RMSNorm case has at
# least 4096 elements for this reason.  The RoPE cases are as small as their paths allow (S2 has 120 elements), so
# their mismatches are pooled: over the pair layouts, table types and append modes of one case, and over the cases
# of one kernel.  The DISTANCE cap holds for every element of every run; a share is asserted on every pool of at
# least SHARE_MIN_ELEMENTS (every case but S2, and both kernels with S2 among the scalar one's cases).
SHARE_MIN_ELEMENTS = 4096


class Pool:
    """mismatch counts of several comparisons taken together"""

    def __init__(self):
        self.bad, self.n, self.dist = 0, 0, 0

    def add(self, got_bits, ref_bits):
        d = t_ulp_distance(got_bits, ref_bits)
        self.bad, self.n, self.dist = self.bad + int((d != 0).sum()), self.n + d.size, max(self.dist, int(d.max()))

    def merge(self, other):
        self.bad, self.n, self.dist = self.bad + other.bad, self.n + other.n, max(self.dist, other.dist)

    @property
    def share(self):
        return self.bad / max(self.n, 1)

    def __str__(self):
        return "%d of %d elements differ (share %.5f), distance %d" % (self.bad, self.n, self.share, self.dist)

    def check(self, cap, what):
        assert self.dist <= cap[1], (what, str(self), "distance cap %d" % cap[1])
        if self.n >= SHARE_MIN_ELEMENTS:
            assert self.share <= cap[0], (what, str(self), "share cap %.5f" % cap[0])


# ---- references -------------------------------------------------------------------------------------------------
def rms_norm_ref(x_T, w_T, eps, res_T=None, *, bits):
    """x_T [tokens, dim], w_T [dim], res_T like x_T or None: values of T (any float array).  Returns (out bits,
    residual-out bits or None).  h = x + res is exact in float64; the kernel normalises its fp32 h, not T(h)."""
    h = np.asarray(x_T, np.float64)
    res_out = None
    if res_T is not None:
        h = h + np.asarray(res_T, np.float64)
        res_out = f64_to_t_bits(h, bits)
    rs = 1.0 / np.sqrt((h * h).mean(axis=-1, keepdims=True) + np.float64(np.float32(eps)))
    out = f64_to_t_bits(round_to_t(h * rs, bits) * np.asarray(w_T, np.float64), bits)
    return out, res_out


def silu_mul_f64(x_T):
    x = np.asarray(x_T, np.float64)
    d = x.shape[-1] // 2
    g, u = x[..., :d], x[..., d:]
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g)) * u


def silu_mul_ref(x_T, *, bits):
    """x_T [tokens, 2 d] = [gate | up] -> bits of T(g / (1 + exp(-g)) u)"""
    return f64_to_t_bits(silu_mul_f64(x_T), bits)


def rope_f64(x_T, positions, table, rot_dim, interleaved):
    """x_T [tokens, heads, head_dim]; table [max_pos, rot_dim] = [cos | sin] of the values the kernel is given"""
    x = np.array(x_T, dtype=np.float64)
    table = np.asarray(table, np.float64)
    half = rot_dim // 2
    i0 = 2 * np.arange(half) if interleaved else np.arange(half)
    i1 = i0 + 1 if interleaved else i0 + half
    c = table[np.asarray(positions), :half][:, None, :]
    s = table[np.asarray(positions), half:rot_dim][:, None, :]
    a, b = x[..., i0].copy(), x[..., i1].copy()
    x[..., i0] = a * c - b * s
    x[..., i1] = b * c + a * s
    return x                                                       # dims >= rot_dim pass through


def rope_ref(x_T, positions, table, rot_dim, interleaved, *, bits):
    return f64_to_t_bits(rope_f64(x_T, positions, table, rot_dim, interleaved), bits)


# ---- RoPE on integers: every result exact in bf16 and f16 -------------------------------------------------------
ROPE_XMAX = 3


def exact_rope_table(max_pos, rot_dim):
    """[max_pos, rot_dim] float64 integers in [0, 15]: no two neighbouring rows, pair indices or halves agree, so a
    wrong row, pair, head or column changes bits"""
    p, r = np.arange(max_pos)[:, None], np.arange(rot_dim // 2)[None, :]
    return np.concatenate([(7 * p + 3 * r) % 16, (5 * p + 11 * r + 1) % 16], axis=1).astype(np.float64)


def exact_rope_inputs(seed, n_tokens, n_heads, head_dim):
    """[tokens, heads, head_dim] float64 integers in [-3, 3], no all-zero pair position left to chance: every row
    of head_dim values holds a non-zero"""
    rng = np.random.default_rng([seed, 0x209E])
    x = rng.integers(-ROPE_XMAX, ROPE_XMAX + 1, size=(n_tokens, n_heads, head_dim))
    t, h = np.nonzero(~x.any(axis=2))
    x[t, h, 0] = 1
    return x.astype(np.float64)


def exact_rope_expect(x, positions, table, rot_dim, interleaved):
    """the rotation in integer arithmetic, and its exactness budget: |a c - b s| <= 2 * 3 * 15 = 90 < 256 = 2^8, so
    every product, every sum and every result is an integer that bf16 (8 significant bits), f16 and fp32 hold
    exactly, whatever the order of operations or the use of an fma"""
    xi, ti = np.asarray(x).astype(np.int64), np.asarray(table).astype(np.int64)
    assert np.array_equal(xi, x) and np.array_equal(ti, table) and np.abs(xi).max() <= ROPE_XMAX
    assert ti.min() >= 0 and ti.max() <= 15 and ti.shape[1] == rot_dim
    half = rot_dim // 2
    i0 = 2 * np.arange(half) if interleaved else np.arange(half)
    i1 = i0 + 1 if interleaved else i0 + half
    c, s = ti[np.asarray(positions), :half][:, None, :], ti[np.asarray(positions), half:][:, None, :]
    a, b = xi[..., i0].copy(), xi[..., i1].copy()
    out = xi.copy()
    out[..., i0] = a * c - b * s
    out[..., i1] = b * c + a * s
    assert np.abs(out).max() <= 2 * ROPE_XMAX * 15 < 256
    for bits in BITS:                                              # representable: T(out) == out
        assert np.array_equal(round_to_t(out.astype(np.float64), bits), out)
    return out


# ---- cases: RMSNorm ---------------------------------------------------------------------------------------------
RMS_EPS = 1e-5
RMS_DIM_MAX = 16384
RMS_DIM_UNSUPPORTED = 16392
# (dim, tokens): NV = vectors of 8 columns per thread, 256 threads per row
RMS = [
    (8, 512),        # one vector, 255 clamped threads
    (2048, 3),       # NV1 exactly full
    (2056, 3),       # NV2, the second iteration has one valid vector
    (5120, 3),       # NV4, one partly and one fully masked iteration
    (8200, 3),       # NV8, three masked iterations
    (16384, 2),      # NV8 full, the API limit
]
RMS_INPLACE = (2056, 3)              # out is x


def rms_nv(dim):
    """the NV slm_rms_norm instantiates (csrc/glue.hip, SLM_NORM_NV)"""
    per_thread = (dim // 8 + 255) // 256
    return 1 if per_thread <= 1 else 2 if per_thread <= 2 else 4 if per_thread <= 4 else 8


RMS_NV = {8: 1, 2048: 1, 2056: 2, 5120: 4, 8200: 8, 16384: 8}
assert all(rms_nv(d) == nv for d, nv in RMS_NV.items()) and all(d * t >= 4096 for d, t in RMS)


def _randn_t(rng, shape, bits, scale=1.0):
    """values of T as float64"""
    return round_to_t(scale * rng.standard_normal(shape), bits)


@functools.lru_cache(maxsize=None)
def rms_inputs(bits, dim, tokens, with_res):
    """(x, w, res or None) as values of T.  Row 0 is scaled by 64, row 1 by 2^-10 (mean(h^2) ~ 1e-6 against
    eps = 1e-5: eps-dominated; rounded to T again, as the smallest f16 values become subnormal), row 2 where there
    is one is all zeros; every other row is plain randn."""
    rng = np.random.default_rng([dim, tokens, BITS.index(bits), int(with_res), 0x9157])
    x = _randn_t(rng, (tokens, dim), bits)
    res = _randn_t(rng, (tokens, dim), bits) if with_res else None
    w = round_to_t(1.0 + 0.1 * rng.standard_normal(dim), bits)
    for a in (x, res):
        if a is not None:
            a[0] *= 64.0
            a[1] = round_to_t(a[1] * 2.0 ** -10, bits)             # (f16: the smallest become subnormal)
            if tokens > 2:
                a[2] = 0.0
            assert np.array_equal(round_to_t(a, bits), a)
    for a in (x, w, res):
        if a is not None:
            a.setflags(write=False)
    return x, w, res


@functools.lru_cache(maxsize=None)
def rms_case(bits, dim, tokens, with_res):
    """inputs and the reference, computed once"""
    x, w, res = rms_inputs(bits, dim, tokens, with_res)
    out, res_out = rms_norm_ref(x, w, RMS_EPS, res, bits=bits)
    return x, w, res, out, res_out


# ---- cases: SiLU * mul ------------------------------------------------------------------------------------------
# (tokens, d); 2048 workgroups of 256 threads take one vector of 8 each per grid-stride iteration
SILU = [
    (1, 8),          # a single vector
    (7, 4104),       # d / 8 = 513: no multiple of 256
    (300, 14336),    # 537 600 vectors > 2048 * 256: the second grid-stride iteration; 17 MB of input
]
SILU_GRID_VECTORS = 2048 * 256
assert SILU[2][0] * SILU[2][1] // 8 == 537600 > SILU_GRID_VECTORS >= SILU[1][0] * SILU[1][1] // 8
# planted into row 0: gates (columns 0..) and the up values beside them
SILU_GATES = [0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0]
SILU_UPS = [2.0, -3.0, 0.0, 1.5, 0.5, -0.75, 1.0, -1.0]
SILU_GATE_BF16 = (-1e4, 2.0)         # column 8, bf16 only, where d > 8


def silu_planted(bits, d):
    """[(column, gate, up)]"""
    p = [(i, g, u) for i, (g, u) in enumerate(zip(SILU_GATES, SILU_UPS))]
    if bits == "bf16" and d > 8:
        p.append((8, round_to_t(np.float64(SILU_GATE_BF16[0]), bits).item(), SILU_GATE_BF16[1]))
    return p


@functools.lru_cache(maxsize=None)
def silu_case(bits, tokens, d):
    """(x [tokens, 2 d] as values of T, reference bits)"""
    rng = np.random.default_rng([tokens, d, BITS.index(bits), 0x5111])
    x = _randn_t(rng, (tokens, 2 * d), bits, 3.0)
    for col, g, u in silu_planted(bits, d):
        x[0, col], x[0, d + col] = g, u
    assert np.array_equal(round_to_t(x, bits), x)
    x.setflags(write=False)
    return x, silu_mul_ref(x, bits=bits)


@functools.lru_cache(maxsize=None)
def silu_deep_case(bits):
    """(x [1, 2 * 64], reference bits): gates from -60 down to -107 in steps of 3/4.  Below -87.3 the sigmoid is an
    fp32 subnormal (the hardware reciprocal flushes those) and below -88.7 its exp2 overflows, while silu(g) u is
    still a normal or subnormal bf16 number: silu_mul1 (csrc/common.h) carries the sigmoid times 2^32 there."""
    d = 64
    g = round_to_t(-60.0 - 0.75 * np.arange(d), bits)
    u = np.tile([1.0, -1.5, 64.0, -0.5], d // 4)
    x = np.concatenate([g, u])[None, :]
    assert np.array_equal(round_to_t(x, bits), x)
    x.setflags(write=False)
    want = silu_mul_ref(x, bits=bits)
    if bits == "bf16":                                             # the case means something: non-zero results
        assert ((want & 0x7FFF) != 0).mean() > 0.8                 # below -87.3 too
        assert ((want & 0x7FFF) != 0)[0, g < -89.0].any()
    return x, want


# ---- cases: RoPE + KV append ------------------------------------------------------------------------------------
# layout: "split" = q, k, v are three contiguous tensors; "buf+P" = the [q | k | v] column slices of ONE
# [T, N + P] buffer (how decode calls it; the P padding columns hold the canary)
RopeCase = namedtuple("RopeCase", "name T nh nkv D rot layout path gy")
ROPE = [
    RopeCase("V1", 5, 4, 2, 64, 32, "split", "vector", 1),       # partial rotary
    RopeCase("V2", 3, 16, 4, 128, 128, "split", "vector", 2),    # 448 units
    RopeCase("V4", 3, 32, 8, 128, 128, "split", "vector", 4),    # 896 units
    RopeCase("S1", 5, 3, 1, 80, 20, "split", "scalar", 0),       # rot % 8 = 4
    RopeCase("S1b", 2, 32, 8, 80, 20, "split", "scalar", 0),     # 320 q pairs: the 256-thread loop wraps
    RopeCase("S2", 4, 2, 1, 10, 6, "split", "scalar", 0),        # head_dim % 4 != 0, 2-byte V copy
    RopeCase("S3", 4, 4, 2, 64, 64, "buf+2", "scalar", 0),       # token stride % 4 = 2
    RopeCase("VS", 4, 4, 2, 64, 64, "buf+4", "vector", 1),       # strided views on the vector path
]
ROPE_BY_NAME = {c.name: c for c in ROPE}
ROPE_MAX_POS = 37                    # the table has exactly this many rows; positions reach the last one
ROPE_TABLES = ("f32", "T")


def rope_pad(case):
    return int(case.layout[4:]) if case.layout.startswith("buf+") else 0


def rope_token_strides(case, append):
    """(q, k, v) token strides in elements, as kernels.apply_rotary_pos_emb passes them"""
    if case.layout == "split":
        return case.nh * case.D, case.nkv * case.D, case.nkv * case.D if append else 0
    n = (case.nh + 2 * case.nkv) * case.D + rope_pad(case)
    return n, n, n if append else 0


def rope_dispatch(n_heads, n_kv_heads, head_dim, rot_dim, q_ts, k_ts, v_ts, append, has_table=True,
                  pointers=(0, 0, 0, 0, 0)):
    """("vector", gridDim.y) or ("scalar", 0): the arithmetic of slm_rope_kv_append (csrc/glue.hip) restated -- the
    `vec` predicate, `units` and `gy`.  A change of the thresholds there has to be made here as well; until it is,
    the case table fails instead of losing a path quietly.  pointers: q, k, v, key cache, value cache."""
    vec = (has_table and rot_dim % 8 == 0 and head_dim % 4 == 0 and q_ts % 4 == 0 and k_ts % 4 == 0 and
           (not append or v_ts % 4 == 0) and not any(p & 7 for p in pointers))
    if not vec:
        return "scalar", 0
    units = (n_heads + n_kv_heads) * (rot_dim // 8) + n_kv_heads * head_dim // 4
    return "vector", 4 if units > 768 else 2 if units > 256 else 1


def rope_case_dispatch(case, append, pointers=(0, 0, 0, 0, 0)):
    return rope_dispatch(case.nh, case.nkv, case.D, case.rot, *rope_token_strides(case, append), append,
                         pointers=pointers)


for _c in ROPE:                      # every named path is reached, with and without the append
    for _append in (True, False):
        assert rope_case_dispatch(_c, _append) == (_c.path, _c.gy), (_c, _append)
assert ROPE_BY_NAME["S1b"].nh * ROPE_BY_NAME["S1b"].rot // 2 > 256


def rope_n_slots(case):
    """used slots include 0 and n_slots - 1 and one token has slot -1: a case of two tokens has ONE slot (token 0
    in slot 0 = n_slots - 1, token 1 skipped); every other case leaves slots unused between the used ones"""
    return 1 if case.T < 3 else 2 * case.T + 3


@functools.lru_cache(maxsize=None)
def rope_index(name):
    """(positions [T] int32 with 0 and max_pos - 1 among them, slot ids [T] int32 with 0, n_slots - 1 and one -1)"""
    case = ROPE_BY_NAME[name]
    rng = np.random.default_rng([ROPE.index(case), 0x1D5])
    pos = rng.integers(0, ROPE_MAX_POS, size=case.T)
    pos[[0, case.T - 1]] = [ROPE_MAX_POS - 1, 0]
    n_slots = rope_n_slots(case)
    if case.T < 3:
        slots = np.array([0, -1])
    else:
        inner = rng.permutation(np.arange(1, n_slots - 1))[:case.T - 3]
        slots = rng.permutation(np.concatenate([[0, n_slots - 1, -1], inner]))
    pos, slots = pos.astype(np.int32), slots.astype(np.int32)
    assert {0, ROPE_MAX_POS - 1} <= set(pos.tolist()) and 0 <= pos.min() and pos.max() < ROPE_MAX_POS
    used = slots[slots >= 0]
    assert (slots == -1).sum() == 1 and {0, n_slots - 1} <= set(used.tolist()) and used.max() < n_slots
    assert np.unique(used).size == used.size == case.T - 1 and slots.min() == -1
    pos.setflags(write=False)
    slots.setflags(write=False)
    return pos, slots


def real_rope_table(rot_dim, table, bits):
    """[max_pos, rot_dim] float64: cos | sin of p * 10000^(-2 i / rot) evaluated in float64, then rounded to what
    the kernel is given (fp32 or T)"""
    inv = 1.0 / 10000.0 ** (np.arange(0, rot_dim, 2, dtype=np.float64) / rot_dim)
    ang = np.arange(ROPE_MAX_POS, dtype=np.float64)[:, None] * inv[None, :]
    t = np.concatenate([np.cos(ang), np.sin(ang)], axis=1)
    return t.astype(np.float32).astype(np.float64) if table == "f32" else round_to_t(t, bits)


@functools.lru_cache(maxsize=None)
def rope_exact_case(name, interleaved):
    """(q, k, v, table, q expectation, k expectation): float64 integers, the same for both dtypes and table types"""
    case = ROPE_BY_NAME[name]
    seed = 10 * ROPE.index(case)
    q = exact_rope_inputs(seed, case.T, case.nh, case.D)
    k = exact_rope_inputs(seed + 1, case.T, case.nkv, case.D)
    v = exact_rope_inputs(seed + 2, case.T, case.nkv, case.D)
    table = exact_rope_table(ROPE_MAX_POS, case.rot)
    pos, _ = rope_index(name)
    out = (q, k, v, table, exact_rope_expect(q, pos, table, case.rot, interleaved),
           exact_rope_expect(k, pos, table, case.rot, interleaved))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rope_real_case(name, interleaved, table, bits):
    """(q, k, v, table as given to the kernel, q reference bits, k reference bits); q, k, v are randn values of T"""
    case = ROPE_BY_NAME[name]
    rng = np.random.default_rng([ROPE.index(case), BITS.index(bits), 0x20BE])
    q = _randn_t(rng, (case.T, case.nh, case.D), bits)
    k = _randn_t(rng, (case.T, case.nkv, case.D), bits)
    v = _randn_t(rng, (case.T, case.nkv, case.D), bits)
    tab = real_rope_table(case.rot, table, bits)
    pos, _ = rope_index(name)
    out = (q, k, v, tab, rope_ref(q, pos, tab, case.rot, interleaved, bits=bits),
           rope_ref(k, pos, tab, case.rot, interleaved, bits=bits))
    for a in out:
        a.setflags(write=False)
    return out
