"""Case lists of the exact int4 GEMM tests: what tests/test_w4_exact_gpu.py runs on the device and what
tests/test_w4_exact_cpu.py checks the recipe on (budget, density, both dequant forms emulated in fp32) without one.

Shapes are the smallest at which each kernel's mechanisms still exist; they come from the grids of test_w4_gpu.py,
test_w4_silu_gpu.py, test_w8_gpu.py and test_moe_gpu.py with K cut to the exactness budget of
helpers.assert_exact_budget: K <= 4096 with |x| <= 2 and scales {1/4, 1/2, 1} in bf16, K <= 2048 with |x| <= 1 and
scales {1/2, 1} in f16 (the magic number 1024 eats the rest).  A biased case takes a small bias in bf16 and a "big"
one in f16 (helpers.exact_bias), so that f16 outputs need rounding too.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

from tests import helpers

BITS = ("bf16", "f16")
K_MAX = {"bf16": 4096, "f16": 2048}

# knobs: tuning of this one case on top of its group's
Case = namedtuple("Case", "M N K gs fmt act bias knobs")
# kernel / row_tiles: what slm_w4a16_gemm_plan must answer for every case of the group (None: not pinned)
Group = namedtuple("Group", "name kernel row_tiles knobs cases")


def _c(M, N, K, gs, fmt, act=False, bias=False, **knobs):
    return Case(M, N, K, gs, fmt, act, bias, knobs)


def _alt_bias(cases, first=True):
    """bias on every other case, as the grids of test_w4_gpu.py do"""
    return [c._replace(bias=(i % 2 == 0) == first) for i, c in enumerate(cases)]


def seed_of(name, index=0):
    return (zlib.crc32(name.encode()) % 100000) * 100 + index


# ---- GEMV (w4_gemv.hip), forced for M <= 4 ----------------------------------------------------------------------
GEMV = Group("GEMV", "GEMV", 0, dict(SLM_W4_GEMV=2), [
    _c(1, 64, 128, 128, "awq"),
    _c(1, 224, 1792, 256, "gptq"),             # K no multiple of the 8-way slicing, group wider than a slice
    _c(3, 96, 1152, 64, "gptq", act=True),
    _c(4, 384, 2048, -1, "gptq"),              # per-channel: a K slice holds part of a group
    _c(4, 288, 2048, 128, "awq", bias=True)])
# the cross-workgroup split of a deferred call: (M, N, K, knobs), group 128, AWQ; the fp32 slabs must sum to the
# truth.  A split keeps >= 4 64-deep chunks per in-workgroup slice: at f16's K = 2048 that needs 4 slices, not 8.
GEMV_DEFERRED = {"bf16": (1, 4096, 4096, {}), "f16": (1, 4096, 2048, dict(SLM_W4_GEMV_KS=4))}

# ---- K-sliced stream, one row tile (w4_ks.hip) ------------------------------------------------------------------
KS1 = Group("KS1", "KS", 1, dict(SLM_W4_KS=1), _alt_bias([
    _c(17, 512, 2048, 128, "gptq", SLM_W4_KS_CW=1),                                   # 2 workgroups over K
    _c(5, 288, 1152, 64, "gptq", act=True, SLM_W4_KS_CW=2, SLM_W4_KS_NW=4),           # 9 chunks on 4 x 2
    _c(32, 160, 640, 32, "gptq", SLM_W4_KS_CW=2),                                     # group 32, idle waves
    _c(8, 384, 2048, -1, "gptq", SLM_W4_KS_CW=4, SLM_W4_KS_NW=4),                     # per-channel
    _c(2, 224, 1792, 256, "gptq", SLM_W4_KS_CW=1, SLM_W4_KS_TPW=2),                   # group > slice
    _c(32, 2048, 1024, 128, "awq", SLM_W4_KS_NW=4, SLM_W4_KS_CW=2, SLM_W4_KS_TPW=5),  # ragged tile runs
    _c(24, 96, 512, 128, "awq")]))                                                    # 4 chunks: 4-wave workgroup

# ---- K-sliced stream, two row tiles -----------------------------------------------------------------------------
KS2 = Group("KS2", "KS", 2, dict(SLM_W4_KS_MT2=1), _alt_bias([
    _c(40, 1024, 1152, 128, "gptq"),                       # 9 chunks: 7 idle waves in slab 2
    _c(64, 480, 1024, 128, "gptq", SLM_W4_KS_TPW=4),       # 15 tiles in runs of 4
    _c(50, 384, 2048, -1, "gptq"),                         # per-channel
    _c(57, 224, 1792, 256, "gptq", SLM_W4_KS_TPW=2),       # group wider than a wave's chunk
    _c(64, 2048, 2048, 128, "gptq", act=True),             # act-order column gather
    _c(34, 96, 128, 128, "awq"),                           # one chunk: 7 idle waves
    _c(33, 640, 2048, 128, "awq"),                         # one live row in the second tile
    _c(48, 256, 2048, 128, "awq", SLM_W4_KS_MT2=2)]))      # the deep form's knob

# ---- lean small-M kernel (w4_small.hip) -------------------------------------------------------------------------
# (K, N, group) of test_moe_gpu.STREAM_CASES (the main loop it shares with the grouped kernel), at expert 0's rows
STREAM_SHAPES = [(17, 256, 192, 128), (32, 640, 64, 32), (9, 640, 128, 64), (3, 1024, 64, 256), (6, 384, 64, 384),
                 (8, 256, 128, 128)]
_SMALL_CASES = _alt_bias([_c(17, 512, 2048, 64, "gptq"), _c(8, 384, 2048, -1, "gptq", act=True),
                          _c(2, 160, 640, 32, "gptq")] +
                         [_c(M, N, K, gs, ("awq", "gptq")[i % 2]) for i, (M, K, N, gs) in enumerate(STREAM_SHAPES)],
                         first=False)
SMALL = [Group("SMALL-sk%d" % sk, "SMALL", 1, dict(SLM_W4_KS=0, SLM_W4_SPLITK=sk), _SMALL_CASES) for sk in (1, 3)]

# ---- general kernel (w4_general.hip) ----------------------------------------------------------------------------
_GENERAL_M64 = _alt_bias([_c(33, 96, 640, 32, "awq"), _c(64, 160, 1152, 64, "gptq", act=True),
                          _c(50, 256, 2048, 128, "awq"), _c(40, 384, 1024, -1, "gptq")], first=False)
_GENERAL_M128 = _alt_bias([_c(100, 160, 640, 32, "awq"), _c(65, 96, 1152, 64, "gptq", act=True),
                           _c(128, 256, 2048, 128, "awq"), _c(111, 384, 1024, -1, "gptq")])


def general_groups():
    """(row tiles, POST, PC, SPLITK): 33 <= M <= 64 without the two-row-tile stream, 65 <= M <= 128 without
    w4_m128.hip on 2 and 4 row tiles.  Four row tiles have no post-scaled form and stage one chunk per pass."""
    out = []
    for mode, mt, base, cases in (("m64", 2, dict(SLM_W4_KS_MT2=0), _GENERAL_M64),
                                  ("mt2", 2, dict(SLM_W4_M128=0, SLM_W4_MT=2), _GENERAL_M128),
                                  ("mt4", 4, dict(SLM_W4_M128=0, SLM_W4_MT=4), _GENERAL_M128)):
        for post in ((0, 1) if mt < 4 else (0,)):
            for pc in ((1, 2, 4) if mt < 4 else (1,)):
                for sk in (0, 3, 7):
                    out.append(Group("GENERAL-%s-post%d-pc%d-sk%d" % (mode, post, pc, sk), "GENERAL", mt,
                                     dict(base, SLM_W4_POST=post, SLM_W4_PC=pc, SLM_W4_SPLITK=sk), cases))
    return out


def general_variant(case, mt, post, pc):
    """{row tiles, column tiles per wave, chunks per pass, post} the plan must report: PC * MT <= 4 in whole
    divisors of the chunk count; the post-scaled form where w4_post_fits (csrc/w4_common.h) says it exists.
    This restates the general kernel's planner (its PC clamp and w4_post_fits) so that the test owns an expectation
    instead of echoing the plan: a change to either in csrc/ has to be made here as well, and until it is, the
    plan assertion of every GENERAL group fails."""
    if pc * mt > 4:
        pc = 1 if mt >= 4 else 4 // mt
    while pc > 1 and (case.K // 128) % pc:
        pc >>= 1
    fits = mt <= 2 and not (case.gs == 32 and (mt == 2 or pc >= 2))
    return [mt, 1, pc, int(bool(post) and fits)]


# ---- w4_m128.hip ------------------------------------------------------------------------------------------------
M128_VARIANTS = [(2, 1, 4, 0), (4, 1, 4, 0), (2, 2, 4, 0), (4, 2, 4, 0), (2, 1, 8, 0), (4, 1, 8, 0), (2, 1, 8, 1),
                 (4, 1, 8, 1)]  # (wd, kw, ct, adma) of test_m128_kernel_grid
_M128_CASES = _alt_bias([
    _c(65, 128, 128, 128, "awq"), _c(128, 256, 512, 128, "gptq"), _c(100, 160, 640, 32, "awq"),
    _c(96, 96, 1152, 64, "gptq", act=True), _c(127, 384, 2048, -1, "gptq"),
    _c(128, 256, 1024, 128, "awq", SLM_W4_SPLITK=2), _c(80, 224, 1792, 128, "gptq", SLM_W4_SPLITK=7),
    _c(66, 128, 4096, 128, "awq", SLM_W4_SPLITK=4), _c(128, 4096, 1024, 32, "gptq", act=True, SLM_W4_SPLITK=3),
    _c(111, 512, 896, 64, "awq")])


def m128_group(wd, kw, ct, adma):
    return Group("M128-wd%d-kw%d-ct%d-adma%d" % (wd, kw, ct, adma), "M128", 4,
                 dict(SLM_W4_M128=1, SLM_W4_M128_WD=wd, SLM_W4_M128_KW=kw, SLM_W4_M128_CT=ct, SLM_W4_M128_ADMA=adma,
                      SLM_W4_SPLITK=0), _M128_CASES)


# ---- w4_ws.hip / w4_xl.hip, forced on small problems ------------------------------------------------------------
def _large_cases(n0, n_last):
    return _alt_bias([
        _c(129, n0, 128, 128, "awq"), _c(256, 2 * n0, 512, 128, "gptq"), _c(300, 160, 640, 32, "awq"),
        _c(200, 96, 1152, 64, "gptq", act=True), _c(257, 384, 2048, -1, "gptq"),
        _c(512, 256, 1024, 128, "awq", SLM_W4_SPLITK=2), _c(256, 224, 1792, 128, "gptq", SLM_W4_SPLITK=7),
        _c(130, n_last, 4096, 128, "awq", SLM_W4_SPLITK=4)])


WS = Group("WS", "WS", 8, dict(SLM_W4_MT=8, SLM_W4_SPLITK=0), _large_cases(128, 128))
XL = Group("XL", "XL", 8, dict(SLM_W4_MT=16, SLM_W4_SPLITK=0), _large_cases(256, 288))

# ---- stream-K form of w4_xl.hip: >= 128 tiles of 256 x 256, N % 256 == 0, an even chunk count --------------------
# forms a case runs in: (name, knobs, kernel the plan must answer).  SLM_W4_XL_SK=0 alone is "the tile form" of the
# default plan, which at these N is the 256 x 128 wave-specialised kernel; with 16 row tiles forced it is the
# 256 x 256 kernel itself, one tile per workgroup -- the other form of the kernel the stream-K form lives in.
XL_SK_FORMS = [("stream-K", dict(SLM_W4_XL_SK=2), "XL_SK"), ("tiles", dict(SLM_W4_XL_SK=0), "WS"),
               ("tiles-256x256", dict(SLM_W4_XL_SK=0, SLM_W4_MT=16), "XL")]
XL_SK = [_c(1800, 4096, 256, 128, "awq"), _c(1793, 4096, 512, 32, "gptq"), _c(2304, 4096, 1024, 64, "awq", bias=True),
         _c(2049, 4096, 768, -1, "gptq")]

# ---- act-order row-parallel shards: (world, M, N, K, group) -----------------------------------------------------
SHARDS = [(2, 24, 256, 1024, 128), (4, 24, 256, 1024, 128), (2, 5, 160, 2048, 64), (4, 5, 160, 2048, 64)]

# ---- strided A / C: one case each of KS, GENERAL and WS ---------------------------------------------------------
STRIDED = [Group("strided-KS", "KS", 1, dict(SLM_W4_KS=1), [_c(17, 160, 640, 64, "gptq", bias=True)]),
           Group("strided-GENERAL", "GENERAL", 2, dict(SLM_W4_KS_MT2=0), [_c(50, 96, 1152, 128, "awq")]),
           Group("strided-WS", "WS", 8, dict(SLM_W4_MT=8), [_c(300, 160, 640, 32, "awq", bias=True)])]

# ---- SiLU * mul epilogue: every row of test_w4_silu_gpu.PLANS whose K fits the budget ----------------------------
# (kernel, row tiles or None, knobs, M, N, K, group) in PLANS' order; the format alternates down the list and two rows in
# three carry a bias, so that every kernel has a biased row in both dtypes.  The
# K = 4096 rows run in bf16 only, as in the dense grids.  One row of PLANS is left out: (128, K = 8192, N = 1024)
# under the default plan, whose point is that K >= 8192 keeps the general kernel -- no K inside the budget reaches
# that branch of the planner, and the general kernel's epilogue is covered by the rows that force it.
_SILU_ROWS = [
    ("GEMV", None, dict(SLM_W4_GEMV_KS=4), 1, 512, 1024, 128),                    # 2 tiles x 4 K slices
    ("GEMV", None, dict(SLM_W4_GEMV_KS=2), 1, 1024, 4096, 128),                   # 4 tiles x 2 K slices
    ("GEMV", None, dict(SLM_W4_GEMV=2, SLM_W4_GEMV_KS=4), 3, 256, 512, 32),       # four rows, group 32
    ("KS", 1, dict(SLM_W4_SPLITK=1), 8, 512, 1024, 128),
    ("KS", 1, dict(SLM_W4_SPLITK=1), 32, 512, 1024, 64),
    ("KS", 1, dict(), 17, 256, 2048, 128),                                        # 16 chunks on 8 waves x 2
    ("KS", 1, dict(SLM_W4_SPLITK=4), 32, 1024, 4096, 128),                        # 4 workgroups over K: fused reduce
    ("GENERAL", None, dict(SLM_W4_SMALL=0, SLM_W4_SPLITK=1), 24, 512, 1024, 128),                # one row tile (POST)
    ("GENERAL", None, dict(SLM_W4_SMALL=0, SLM_W4_SPLITK=1, SLM_W4_NTW=2), 24, 512, 1024, 128),  # pair inside a wave
    ("KS", 2, dict(SLM_W4_SPLITK=1), 48, 512, 1024, 128),                         # the default for 33 <= M <= 64
    ("KS", 2, dict(SLM_W4_KS_MT2=1), 48, 512, 1024, 128),                         # in-kernel pair
    ("KS", 2, dict(SLM_W4_KS_MT2=1), 64, 1024, 4096, 128),                        # ... over 4 workgroups
    ("KS", 2, dict(SLM_W4_KS_MT2=1, SLM_W4_KS_TPW=4), 33, 448, 2048, 128),        # ragged runs, one row in tile 2
    ("GENERAL", None, dict(SLM_W4_SPLITK=2), 64, 512, 1024, 32),
    ("GENERAL", None, dict(SLM_W4_MT=4, SLM_W4_SPLITK=1), 100, 512, 1024, 128),   # four row tiles (PRE)
    ("GENERAL", None, dict(SLM_W4_MT=4, SLM_W4_SPLITK=2), 128, 1024, 2048, 128),
    ("WS", None, dict(SLM_W4_MT=8, SLM_W4_SPLITK=1), 256, 1024, 1024, 128),
    ("WS", None, dict(SLM_W4_MT=8, SLM_W4_SPLITK=1), 300, 1152, 1024, 64),        # ragged M, 9 column tiles
    ("WS", None, dict(SLM_W4_MT=8, SLM_W4_SPLITK=2), 256, 1024, 2048, 128),
    ("XL", None, dict(SLM_W4_MT=16, SLM_W4_SPLITK=1), 256, 1024, 1024, 128),
    ("XL", None, dict(SLM_W4_MT=16, SLM_W4_SPLITK=1), 384, 1280, 1024, 128),
    (None, None, dict(), 256, 2048, 4096, 128),                                   # whatever the plan picks
    ("M128", None, dict(SLM_W4_M128=1), 128, 1024, 2048, 128),                    # the plan's split
    ("M128", None, dict(SLM_W4_M128=1, SLM_W4_SPLITK=1), 100, 512, 1024, 32),     # two scale groups per chunk
    ("M128", None, dict(SLM_W4_M128=1, SLM_W4_SPLITK=4), 96, 1024, 4096, 64),     # fp32 slabs + the fused reduce
    ("M128", None, dict(SLM_W4_M128=1, SLM_W4_M128_WD=4, SLM_W4_SPLITK=1), 128, 512, 1024, 128),   # four-chunk ring
    ("M128", None, dict(SLM_W4_M128=1, SLM_W4_SPLITK=1), 65, 448, 1024, 128),     # 7 tile pairs: a clamped wave pair
    ("M128", None, dict(SLM_W4_M128=1, SLM_W4_M128_KW=2, SLM_W4_SPLITK=1), 128, 1024, 2048, 128),  # 2 waves per tile
    ("M128", None, dict(SLM_W4_M128=1, SLM_W4_M128_KW=2, SLM_W4_SPLITK=2), 100, 448, 1024, 32),    # + slabs, clamped
    ("M128", None, dict(SLM_W4_M128=1, SLM_W4_M128_KW=1, SLM_W4_SPLITK=1), 96, 512, 1024, 64),
    ("M128", None, dict(SLM_W4_M128=1, SLM_W4_M128_CT=8, SLM_W4_SPLITK=1), 128, 1024, 2048, 128),  # 256-column groups
    ("M128", None, dict(SLM_W4_M128=1, SLM_W4_M128_CT=8, SLM_W4_SPLITK=2), 100, 448, 1024, 32),
    ("M128", None, dict(SLM_W4_M128=1, SLM_W4_M128_CT=8, SLM_W4_M128_WD=4), 65, 1216, 1024, 128),  # 19 tile pairs
    ("M128", None, dict(SLM_W4_M128=1, SLM_W4_M128_CT=8, SLM_W4_M128_ADMA=1, SLM_W4_SPLITK=1), 128, 1024, 2048, 128),
    ("M128", None, dict(SLM_W4_M128=1, SLM_W4_M128_CT=8, SLM_W4_M128_ADMA=1, SLM_W4_SPLITK=2), 100, 448, 1024, 32),
    ("SMALL", None, dict(SLM_W4_KS=0, SLM_W4_SPLITK=1), 8, 512, 1024, 128),       # pair exchange in LDS
    ("SMALL", None, dict(SLM_W4_KS=0), 17, 256, 2048, 128),                       # split-K -> fused reduce
    ("GENERAL", 2, dict(SLM_W4_KS_MT2=0, SLM_W4_SPLITK=1), 48, 512, 1024, 128),   # two row tiles (POST)
]
SILU = [Group("silu%02d-%s" % (i, kernel or "default"), kernel, row_tiles, knobs,
              [_c(M, N, K, gs, ("awq", "gptq")[i % 2], bias=i % 3 != 0)])
        for i, (kernel, row_tiles, knobs, M, N, K, gs) in enumerate(_SILU_ROWS)]

# ---- 8-bit layers (two int4 planes over 2K rows) through the default plan ---------------------------------------
# M -> the kernels the default plan picks there (M = 48: the two-row-tile stream is built for groups >= 128 only)
W8_M = {1: ("GEMV",), 17: ("KS",), 48: ("KS", "GENERAL"), 100: ("GENERAL",), 200: ("GENERAL",)}
# (N, K, group, format, act-order, symmetric, scale exponent, share of non-zero activations or None)
W8_CASES = {
    "bf16": [(160, 512, 128, "gptq", False, False, 0, None), (96, 256, 64, "awq", False, False, -1, None),
             (128, 512, 32, "gptq", False, True, 1, None), (64, 256, 64, "gptq", True, False, 0, None)],
    "f16": [(160, 128, 128, "gptq", False, False, 0, None), (96, 256, 64, "awq", False, False, -1, 0.4),
            (128, 256, 32, "gptq", False, True, 1, 0.4), (64, 128, 64, "gptq", True, False, 0, None)],
}

assert len(W8_CASES["bf16"]) == len(W8_CASES["f16"])
W8_N = len(W8_CASES["bf16"])

# ---- grouped MoE GEMM: (T, k, K, N, group), E = 8 ---------------------------------------------------------------
MOE_E = 8
MOE = [(1, 2, 256, 192, 128), (33, 2, 384, 128, 32), (96, 4, 640, 320, 64), (3, 1, 128, 64, -1)]
MOE_ROW_SCALES = (0.25, 0.5, 1.0, 2.0)


def dense_groups():
    """every group that runs plain gptq_gemm calls into a contiguous c"""
    return ([GEMV, KS1, KS2] + SMALL + general_groups() + [m128_group(*v) for v in M128_VARIANTS] + [WS, XL])


def cases_of(group, bits):
    """the group's cases inside the dtype's K budget"""
    return [c for c in group.cases if c.K <= K_MAX[bits]]


# ---- inputs -----------------------------------------------------------------------------------------------------
def share_of(truth, bits):
    """share of a float64 truth's elements that are not representable in T, i.e. that the kernel has to round"""
    t32 = truth.astype(np.float32)
    return float((helpers._from_t_bits(helpers._t_bits(t32, bits), bits) != t32).mean())


def assert_share(bits, K, biased, share, what):
    """the rounding of the epilogue and its ties are exercised: some output is not representable in T in every bf16
    case with K >= 512 and in every f16 case with the (big) bias.  Asserted wherever a truth is used, on the CPU
    and on the device, so that a reseeded or reshaped case cannot quietly lose it."""
    if (bits == "bf16" and K >= 512) or (bits == "f16" and biased):
        assert share > 0, what


# the groups that run one shape under other knobs come one after the other (the 18 knob tuples of the general
# kernel over 4 shapes, the 8 forms of w4_m128.hip over 10), in both dtypes: 24 entries hold the widest such run.
# The stream-K cases (thousands of rows: float64 truths of tens of MB) are used once each and are not kept.
_CACHED_ROWS_MAX = 512


def _make_inputs(bits, M, N, K, gs, fmt, act, bias, seed):
    q = helpers.make_exact_quant_case(seed, K, N, gs, fmt, bits, act_order=act)
    a = helpers.exact_activations(seed, M, K, helpers.EXACT_XMAX[bits])
    b = helpers.exact_bias(seed, N, q, big=(bits == "f16")) if bias else None
    helpers.assert_exact_budget(a, q, b)
    truth, share = helpers.exact_truth(a, q, b)
    return q, a, b, truth, share


_inputs = functools.lru_cache(maxsize=24)(_make_inputs)


def inputs(bits, case):
    """(quant case, activations [M, K] fp32, bias [N] fp32 or None, float64 truth, share of outputs that need
    rounding) of one case; the budget and density rules are asserted here, once, for whoever uses the case.
    The inputs depend on the shape alone, not on the knobs: groups that run one shape under other knobs share
    them (and the truth, computed once)."""
    make = _inputs if case.M <= _CACHED_ROWS_MAX else _make_inputs
    return make(bits, *case[:7], shape_seed(case))


def shape_seed(case):
    """one seed per shape: the groups that run the same shapes under other knobs share inputs and truth"""
    return seed_of("%d-%d-%d-%d-%s-%d-%d" % (case.M, case.N, case.K, case.gs, case.fmt, case.act, case.bias))


def inputs8(bits, n, M):
    N, K, gs, fmt, act, sym, exp, nonzero = W8_CASES[bits][n]
    seed = seed_of("w8-%s" % bits, 10 * n)
    q = helpers.make_exact_quant8_case(seed, K, N, gs, fmt, bits, act_order=act, sym=sym, scale_exps=(exp,))
    a = helpers.exact_activations(seed + M, M, K, helpers.EXACT_XMAX[bits], nonzero=nonzero)
    b = helpers.exact_bias(seed + M, N, q, big=(bits == "f16")) if M % 2 else None
    helpers.assert_exact_budget(a, q, b)
    truth, share = helpers.exact_truth(a, q, b)
    return q, a, b, truth, share


def moe_inputs(bits, n):
    """experts (quant cases), routing ids [T, k], activations for a_div = k ([T, K]) and a_div = 1 ([T k, K])"""
    T, k, K, N, gs = MOE[n]
    fmt = ("awq", "gptq")[(n + (bits == "f16")) % 2]
    seed = seed_of("moe-%s" % bits, 100 * n)
    experts = [helpers.make_exact_quant_case(seed + e, K, N, gs, fmt, bits) for e in range(MOE_E)]
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation(MOE_E)[:k] for _ in range(T)]).astype(np.int32)
    a_tok = helpers.exact_activations(seed, T, K, helpers.EXACT_XMAX[bits])
    a_flat = helpers.exact_activations(seed + 1, T * k, K, helpers.EXACT_XMAX[bits])
    row_scale = rng.choice(np.asarray(MOE_ROW_SCALES, np.float32), size=T * k)
    for q in experts:
        helpers.assert_exact_budget(a_tok, q)
        helpers.assert_exact_budget(a_flat, q)
    return experts, ids, a_tok, a_flat, row_scale


def moe_truth(experts, ids, a, a_div):
    """float64 [T k, N]: flat row f = (token f // k, choice f % k) through its expert"""
    flat = ids.reshape(-1)
    w = [helpers._exact_weight(q) for q in experts]
    out = np.zeros((flat.size, experts[0]["N"]), np.float64)
    for f, e in enumerate(flat):
        out[f] = np.asarray(a[f // a_div], np.float64) @ w[e]
    return out


def paired_src_cols(N):
    """checkpoint column of every packed column of a paired [gate | up] weight (SLM_W4_PAIRED: 32-column tiles of
    the two halves interleaved) -- the order a fused call takes its bias in"""
    n = np.arange(N)
    return (n >> 6) * 32 + (n & 31) + np.where(n & 32, N // 2, 0)


def shard_case(q, rank, world):
    """rank's row-parallel shard of an act-order layer: its checkpoint rows and THEIR g_idx, the full scale and
    zero tables (qlinear_gptq_marlin_impl.cpp:236-243,270-276)"""
    ks = q["K"] // world
    rows = slice(rank * ks, (rank + 1) * ks)
    return dict(q, K=ks, q=q["q"][rows], g_idx=q["g_idx"][rows], qweight=q["qweight"][rank * ks // 8:(rank + 1) * ks // 8])


def shard_truths(q, a, world):
    """float64 partial sum of every rank"""
    ks = q["K"] // world
    w = helpers._exact_weight(q)
    return [np.asarray(a[:, r * ks:(r + 1) * ks], np.float64) @ w[r * ks:(r + 1) * ks] for r in range(world)]


def check_xl_plan(case, kernel, plan):
    """one form of XL_SK_FORMS: 256-row blocks (8 row tiles of 32), K unsplit -- the stream-K form cuts the
    tile x K work list, not K -- and for the stream-K form the length of a workgroup's range: the list of
    (256 x 256 tiles) x (128-deep chunks) in 256 equal ranges of whole chunk pairs (plan_xl_sk, w4_plan.hip)"""
    what = (case[:7], kernel, plan.kernel_name, plan.row_tiles, plan.split_k, list(plan.variant))
    assert plan.kernel_name == kernel and plan.row_tiles == 8 and plan.split_k == 1, what
    assert plan.n_mblocks == -(-case.M // 256) and plan.chunks_per_split == case.K // 128, what
    assert plan.n_nblocks == -(-case.N // (256 if kernel != "WS" else 128)), what
    if kernel == "XL_SK":
        per = -(-(plan.n_mblocks * plan.n_nblocks * (case.K // 128)) // 256)
        assert plan.n_mblocks * plan.n_nblocks >= 128 and plan.variant[0] == per + (per & 1), what


def check_shard_plan(k_packed, plan, what):
    """a rank's shard (M <= 24, its rows padded to whole groups of 32): the K-sliced stream on one row tile, and K
    short enough for the waves of ONE workgroup (at most 1536 padded rows: 12 chunks of 128 on chunk waves x
    column waves >= 8), so no slabs"""
    what = (what, plan.kernel_name, plan.row_tiles, plan.split_k, list(plan.variant))
    assert plan.kernel_name == "KS" and plan.row_tiles == 1 and plan.variant[0] == 1, what
    assert plan.split_k == 1 and k_packed // 128 <= plan.variant[1] * plan.variant[2], what


def w8_plan(M, k_packed, group_packed):
    """(kernel, row tiles, split) of the default plan for an 8-bit layer's 2K packed rows: GEMV up to 4 rows, the
    K-sliced stream on one row tile up to 32 and on two up to 64 where the packed group is >= 128 (it is built for
    those only), else the general kernel on two row tiles, which at M <= 64 and a single row of column tiles gives
    every 128-deep chunk to a workgroup of its own.  Restates the planner (w4_plan.hip), as general_variant() does."""
    if M <= 4:
        return "GEMV", 0, 1
    if M <= 32:
        return "KS", 1, 1
    if M <= 64:
        return ("KS", 2, 1) if group_packed >= 128 else ("GENERAL", 2, k_packed // 128)
    return "GENERAL", 2, 1


def check_w8_plan(M, k_packed, group_packed, plan, what):
    got = (plan.kernel_name, plan.row_tiles, plan.split_k)
    assert got == w8_plan(M, k_packed, group_packed) and plan.kernel_name in W8_M[M], (what, got)


# ---- what the plan must say ---------------------------------------------------------------------------------------
def check_plan(group, case, plan):
    """the kernel, row tiles, split and kernel-specific variant slm_w4a16_gemm_plan must answer for a case under
    its group's and its own knobs: a knob that stopped selecting its kernel fails here instead of testing another
    kernel quietly"""
    what = (group.name, case[:7], plan.kernel_name, plan.row_tiles, plan.split_k, list(plan.variant))
    assert group.kernel is None or plan.kernel_name == group.kernel, what
    assert group.row_tiles is None or plan.row_tiles == group.row_tiles, what
    knobs = {**group.knobs, **case.knobs}
    forced = knobs.get("SLM_W4_SPLITK", 0)
    if forced == 1:
        assert plan.split_k == 1, what
    elif forced > 1 and plan.kernel_name != "KS":      # every split the K of the case allows, at most the forced one
        assert 2 <= plan.split_k <= forced, what
    if plan.kernel_name == "KS":
        for i, knob in ((1, "SLM_W4_KS_CW"), (2, "SLM_W4_KS_NW")):
            assert knob not in knobs or plan.variant[i] == knobs[knob], what
        assert plan.variant[0] == plan.row_tiles and plan.split_k == -(-(case.K // 128) // (plan.variant[1] * plan.variant[2])), what
    if group.name.startswith("GENERAL"):
        assert list(plan.variant) == general_variant(case, group.row_tiles, knobs["SLM_W4_POST"], knobs["SLM_W4_PC"]), what
    if group.name.startswith("M128"):
        wd, kw, ct, adma = (knobs["SLM_W4_M128_" + k] for k in ("WD", "KW", "CT", "ADMA"))
        # (the ring falls back to 2 chunks where 4 do not divide a split; 256-column workgroups keep one wave per
        # column tile and are the only form with LDS-DMA activations)
        assert plan.variant[0] in (2, wd) and list(plan.variant[1:]) == [1 if ct == 8 else kw, ct, adma if ct == 8 else 0], what
