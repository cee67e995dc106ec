"""Float64 references, case tables and caps of the Gemma kernels' bit tests: what tests/test_gemma_exact_gpu.py runs on
the device (slm_gemma_norm forms A / B / C and slm_soft_cap: csrc/gemma.hip) and what tests/test_gemma_ref_cpu.py
checks the references and the caps on without one.  Imports no GPU code.

GN(h, w) = T(h rs (1 + w)), rs = 1 / sqrt(mean(h^2) + eps): ONE rounding to T (Gemma's (x (1 + w)).to(T), reference
src/layers/normalization.h:31-40), evaluated here in float64 in the kernel's own order of roundings:
  A  out = GN(x, pre)
  B  y = GN(x, post) (no post weight: y = x); residual = T(y + residual); out = GN(residual, pre)
  C  residual = T(table[id] x_scale); out = GN(residual, pre)
The kernel evaluates the same expressions in fp32 with the hardware's rsq (1 ulp of fp32), so an element may land on
the other side of a rounding boundary of T, by one step, in a small share of elements.  What is compared and the caps
(conditions, not measurements):
  out            against GN of the kernel's OWN residual read back (form A: of x): share <= 0.5 %, distance <= 1 ulp.
  residual, B    every element equals T(y' + residual) for y' = the reference y or one of its two neighbours in T: a
                 one-step flip of y moves a cancelling sum by hundreds of ulps, so a distance on the residual says
                 nothing.  Elements that need a neighbour: <= 0.5 %.
  residual, C    bit-exact: the product of two T values is exact in fp32 and rounded once.
  soft_cap       T(cap tanh(x / cap)): share <= 0.5 %, distance <= 1 ulp, over random logits and planted arguments.

                    cap           | fp32 restatement on the CPU, rsqrt off by 0, +-8 ulps | MI355X (MEASURED)
  out        bf16   0.5 %, 1 ulp  |  0.024 %  1                                            |  0.012 %  1
             f16                  |  0.141 %  1                                            |  0.024 %  1
  residual B bf16   0.5 %, none   |  0.011 %, none outside the three candidates            |  0.002 %  none
             f16                  |  0.098 %, none                                         |  0.006 %  none
  soft_cap   bf16   0.5 %, 1 ulp  |  below half the cap (tests/test_gemma_ref_cpu.py)      |  0.000 %  0
             f16                  |                                                        |  0.029 %  1
The device stays below the restatement because its rsqrt is within one fp32 ulp, not eight.
"""
import functools

import numpy as np

from tests import helpers
from tests.glue_ref import (BITS, CANARY, SHARE_MIN_ELEMENTS, Pool, f64_to_t_bits, round_to_t,  # noqa: F401
                            t_bits_to_f64, t_ulp_distance)

GEMMA_EPS = 1e-6
OUT_CAP = (0.005, 1)                 # share, distance in ulps of T
NEIGHBOUR_CAP = 0.005                # share of form-B residual elements explained only by a neighbour of y
SOFT_CAP_CAP = (0.005, 1)

# share of mismatching elements and largest distance seen on an MI355X (gfx950), worst case per check and dtype;
# "residual": share of elements that needed a neighbour of y, and elements outside the three candidates
MEASURED = {
    ("out", "bf16"): (0.00012, 1), ("out", "f16"): (0.00024, 1),
    ("residual", "bf16"): (0.00002, 0), ("residual", "f16"): (0.00006, 0),
    ("soft_cap", "bf16"): (0.0, 0), ("soft_cap", "f16"): (0.00029, 1),
}

# (dim, tokens): NV = vectors of 8 columns per thread, 256 threads per row; tokens * dim >= 4096
CASES = [
    (8, 512),        # the minimum: one vector, 255 clamped threads
    (2048, 4),       # NV1: one full vector per thread
    (2304, 4),       # NV2, ragged last vector (Gemma-2-2B)
    (3584, 4),       # NV2, ragged (Gemma-2-9B)
    (4608, 4),       # NV4, ragged (Gemma-2-27B)
    (16384, 4),      # NV8 full, the API limit
]
DIM_MAX = 16384
DIM_UNSUPPORTED = (0, 12, 16392)
RESIDUAL_SCALES = (0.125, 1.0, 8.0, 64.0)   # by row % 4: y + residual cancels / is dominated by the residual
SPLITS = (4, 8)
VOCAB = 37
assert all(d * t >= SHARE_MIN_ELEMENTS and t % 4 == 0 for d, t in CASES)


def gemma_nv(dim):
    """the NV slm_gemma_norm instantiates (csrc/gemma.hip, SLM_GN_NV)"""
    per_thread = (dim // 8 + 255) // 256
    return 1 if per_thread <= 1 else 2 if per_thread <= 2 else 4 if per_thread <= 4 else 8


assert [gemma_nv(d) for d, _ in CASES] == [1, 1, 2, 2, 4, 8]


# ---- references -------------------------------------------------------------------------------------------------
def gn_f64(h_T, w_T, eps=GEMMA_EPS):
    """h rs (1 + w) in float64, rows along the last axis; eps as the fp32 value the kernel is given"""
    h = np.asarray(h_T, np.float64)
    rs = 1.0 / np.sqrt((h * h).mean(axis=-1, keepdims=True) + np.float64(np.float32(eps)))
    return h * rs * (1.0 + np.asarray(w_T, np.float64))


def gn_ref(h_T, w_T, eps=GEMMA_EPS, *, bits):
    return f64_to_t_bits(gn_f64(h_T, w_T, eps), bits)


def form_a_ref(x_T, pre_T, eps=GEMMA_EPS, *, bits):
    return gn_ref(x_T, pre_T, eps, bits=bits)


def form_b_ref(x_T, post_T, res_T, pre_T, eps=GEMMA_EPS, *, bits):
    """(out bits or None, residual bits, y bits).  post_T None: y = x; pre_T None: no second stage."""
    y_bits = f64_to_t_bits(x_T, bits) if post_T is None else gn_ref(x_T, post_T, eps, bits=bits)
    r_bits = f64_to_t_bits(t_bits_to_f64(y_bits, bits) + np.asarray(res_T, np.float64), bits)
    out = None if pre_T is None else gn_ref(t_bits_to_f64(r_bits, bits), pre_T, eps, bits=bits)
    return out, r_bits, y_bits


def form_c_ref(table_T, ids, x_scale_T, pre_T, eps=GEMMA_EPS, *, bits):
    """(out bits, residual bits)"""
    r_bits = f64_to_t_bits(np.asarray(table_T, np.float64)[np.asarray(ids)] * np.float64(x_scale_T), bits)
    return gn_ref(t_bits_to_f64(r_bits, bits), pre_T, eps, bits=bits), r_bits


def soft_cap_ref(x_T, cap, *, bits):
    x = np.asarray(x_T, np.float64)
    return f64_to_t_bits(np.float64(cap) * np.tanh(x / np.float64(cap)), bits)


def t_neighbours(u16):
    """(next pattern towards +inf, next towards -inf) of finite T patterns, through zero: -0 and +0 are one value"""
    u = np.asarray(u16).astype(np.uint16).astype(np.int32)
    mag = u & 0x7FFF
    o = np.where(u & 0x8000, -mag, mag)

    def back(v):
        return np.where(v < 0, 0x8000 | (-v), v).astype(np.uint16)
    return back(o + 1), back(o - 1)


def residual_b_explained(got_bits, y_ref_bits, res_T, *, bits):
    """(exact, explained): boolean arrays -- the element equals T(y + residual) for the reference y; for y or one
    of its two neighbours in T"""
    res = np.asarray(res_T, np.float64)

    def hit(yb):
        want = f64_to_t_bits(t_bits_to_f64(yb, bits) + res, bits)
        return t_ulp_distance(got_bits, want) == 0
    up, down = t_neighbours(y_ref_bits)
    exact = hit(y_ref_bits)
    return exact, exact | hit(up) | hit(down)


def check_residual_b(got_bits, y_ref_bits, res_T, what, *, bits):
    """the form-B residual rule; returns (share of elements that needed a neighbour, elements outside)"""
    exact, explained = residual_b_explained(got_bits, y_ref_bits, res_T, bits=bits)
    share, outside = float((~exact).mean()), int((~explained).sum())
    assert outside == 0, (what, "%d elements are T(y' + residual) for no candidate y'" % outside)
    assert share <= NEIGHBOUR_CAP, (what, "share %.5f of cap %.5f need a neighbour of y" % (share, NEIGHBOUR_CAP))
    return share, outside


def check_out(got_bits, own_h_bits, pre_T, what, eps=GEMMA_EPS, *, bits, cap=OUT_CAP):
    """out against GN of the kernel's own residual (form A: x) read back; returns (share, distance)"""
    want = gn_ref(t_bits_to_f64(own_h_bits, bits), pre_T, eps, bits=bits)
    d = t_ulp_distance(got_bits, want)
    share, dist = float((d != 0).mean()), int(d.max())
    assert dist <= cap[1] and share <= cap[0], (what, "share %.5f of cap %.5f" % (share, cap[0]),
                                                "distance %d of cap %d" % (dist, cap[1]))
    return share, dist


# ---- fp32 restatements of the kernel arithmetic (the CPU check of the caps, and the wrong kernels) -----------------
def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _rs_f32(h32, eps, rs_ulps):
    ss = (h32.astype(np.float64) ** 2).sum(axis=-1, keepdims=True).astype(np.float32)
    m = ss * np.float32(1.0 / h32.shape[-1]) + np.float32(eps)
    rs = (1.0 / np.sqrt(m.astype(np.float64))).astype(np.float32)
    for _ in range(abs(rs_ulps)):
        rs = np.nextafter(rs, np.float32(np.inf if rs_ulps > 0 else 0.0), dtype=np.float32)
    return rs


def gn_fp32_bits(h_T, w_T, eps=GEMMA_EPS, rs_ulps=0, *, bits):
    h, w = _f32(h_T), _f32(w_T)
    return helpers._t_bits(h * _rs_f32(h, eps, rs_ulps) * (np.float32(1.0) + w), bits)


def form_b_fp32(x_T, post_T, res_T, pre_T, eps=GEMMA_EPS, rs_ulps=0, *, bits):
    """(out bits, residual bits) of the kernel arithmetic in fp32, its rsqrt off by rs_ulps fp32 ulps"""
    y_bits = f64_to_t_bits(x_T, bits) if post_T is None else gn_fp32_bits(x_T, post_T, eps, rs_ulps, bits=bits)
    r_bits = helpers._t_bits(_f32(t_bits_to_f64(y_bits, bits)) + _f32(res_T), bits)
    return gn_fp32_bits(t_bits_to_f64(r_bits, bits), pre_T, eps, rs_ulps, bits=bits), r_bits


def tanh_fp32(z):
    """csrc/gemma.hip tanh_f32 restated: odd polynomial below |z| = 0.25, (1 - e) / (1 + e) above"""
    z = np.asarray(z, np.float32)
    one = np.float32(1.0)
    z2 = z * z
    p = z2 * np.float32(62.0 / 2835.0) + np.float32(-17.0 / 315.0)
    p = z2 * p + np.float32(2.0 / 15.0)
    p = z2 * p + np.float32(-1.0 / 3.0)
    small = (z * z2) * p + z
    with np.errstate(under="ignore", over="ignore"):
        e = np.exp2(np.abs(z) * np.float32(-2.0 * 1.4426950408889634)).astype(np.float32)
    big = np.copysign((one - e) / (one + e), z).astype(np.float32)
    return np.where(np.abs(z) < np.float32(0.25), small, big).astype(np.float32)


def soft_cap_fp32_bits(x_T, cap, *, bits):
    with np.errstate(over="ignore"):
        return helpers._t_bits(np.float32(cap) * tanh_fp32(_f32(x_T) * (np.float32(1.0) / np.float32(cap))), bits)


# ---- inputs -----------------------------------------------------------------------------------------------------
def _randn_t(rng, shape, bits, scale=1.0):
    return round_to_t(scale * rng.standard_normal(shape), bits)


@functools.lru_cache(maxsize=None)
def norm_inputs(bits, dim, tokens):
    """(x, post, pre, res) as values of T: weights 0.3 N(0,1), x 3 N(0,1), residual row t scaled by
    RESIDUAL_SCALES[t % 4]"""
    rng = np.random.default_rng([dim, tokens, BITS.index(bits), 0x6E44A])
    x = _randn_t(rng, (tokens, dim), bits, 3.0)
    post = _randn_t(rng, (dim,), bits, 0.3)
    pre = _randn_t(rng, (dim,), bits, 0.3)
    scale = np.array(RESIDUAL_SCALES)[np.arange(tokens) % 4][:, None]
    res = round_to_t(scale * rng.standard_normal((tokens, dim)), bits)
    for a in (x, post, pre, res):
        a.setflags(write=False)
    return x, post, pre, res


@functools.lru_cache(maxsize=None)
def norm_case(bits, dim, tokens):
    """inputs and the references of forms A and B, computed once: dict"""
    x, post, pre, res = norm_inputs(bits, dim, tokens)
    out_b, r_b, y_b = form_b_ref(x, post, res, pre, bits=bits)
    return dict(x=x, post=post, pre=pre, res=res, out_a=form_a_ref(x, pre, bits=bits), out_b=out_b, res_b=r_b,
                y_b=y_b)


@functools.lru_cache(maxsize=None)
def slabs_case(bits, dim, tokens, n_splits):
    """(slabs [n_splits, tokens, dim] float32, x = T(their sum) as float64).  Every slab element is a multiple of
    2^-6 below 2^8, so partial sums are multiples of 2^-6 below 2^11: exact in fp32 in any order."""
    rng = np.random.default_rng([dim, tokens, n_splits, BITS.index(bits), 0x51AB])
    k = rng.integers(-(2 ** 14) + 1, 2 ** 14, size=(n_splits, tokens, dim))
    slabs = (k * 2.0 ** -6).astype(np.float32)
    total = k.sum(axis=0) * 2.0 ** -6
    assert np.abs(slabs).max() < 2 ** 8 and np.array_equal(slabs.astype(np.float64).sum(axis=0), total)
    x = round_to_t(total, bits)
    slabs.setflags(write=False)
    x.setflags(write=False)
    return slabs, x


def embed_scale(dim, bits):
    """T(sqrt(hidden)) (gemma2.h:236-238) as float64"""
    return round_to_t(np.array([np.sqrt(dim)]), bits).item()


@functools.lru_cache(maxsize=None)
def embed_case(bits, dim, tokens):
    """(table [VOCAB, dim], ids int32 [tokens] with 0 and VOCAB - 1 among them, x_scale, pre, out bits, res bits)"""
    rng = np.random.default_rng([dim, tokens, BITS.index(bits), 0xE3BED])
    table = _randn_t(rng, (VOCAB, dim), bits, 0.05)
    pre = _randn_t(rng, (dim,), bits, 0.3)
    ids = rng.integers(0, VOCAB, size=tokens).astype(np.int32)
    ids[[0, -1]] = [VOCAB - 1, 0]
    scale = embed_scale(dim, bits)
    out, r = form_c_ref(table, ids, scale, pre, bits=bits)
    for a in (table, pre, ids):
        a.setflags(write=False)
    return table, ids, scale, pre, out, r


# ---- soft cap ---------------------------------------------------------------------------------------------------
SOFT_CAPS = (30.0, 50.0)
SOFT_CAP_SHAPE = (5, 4104)           # 2565 vectors: no multiple of 256, several workgroups
SOFT_CAP_ROW_LEN_UNSUPPORTED = (0, 12, 4100)
SOFT_CAP_PLANTED_Z = [s * 2.0 ** k for k in range(-14, 4, 1) for s in (1.0, -1.0)]   # +-2^-14 ... +-8, steps of 2


def largest_finite(bits):
    return 65504.0 if bits == "f16" else float(np.float32(3.3895313892515355e38))


@functools.lru_cache(maxsize=None)
def soft_cap_case(bits, cap):
    """(x [rows, row_len] as values of T, reference bits, planted columns of row 0): logits 12 N(0,1), and in row 0
    the arguments x = cap z for z = +-2^-14 ... +-8 (exact in T: cap has few bits), 0 and +-the largest finite"""
    rng = np.random.default_rng([BITS.index(bits), int(cap), 0x50F7])
    x = _randn_t(rng, SOFT_CAP_SHAPE, bits, 12.0)
    planted = [cap * z for z in SOFT_CAP_PLANTED_Z] + [0.0, largest_finite(bits), -largest_finite(bits)]
    x[0, :len(planted)] = planted
    assert np.array_equal(round_to_t(x, bits), x)
    x.setflags(write=False)
    return x, soft_cap_ref(x, cap, bits=bits), len(planted)
