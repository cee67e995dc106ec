"""Float64 reference and case table of the QK-norm prologue (include/slm_hip.h section 19: slm_qk_norm_rope_kv_append
and its split-K form), shared by tests/test_qk_norm_ref_cpu.py and tests/test_qk_norm_exact_gpu.py.

The reference is built from the references tests/glue_ref.py already holds for the two kernels the prologue must agree
with bit for bit (RMSNorm: fp32 statistic, T(T(x rs) w); RoPE: one rounding of a c -/+ b s), applied per head: the
norm over each head's D values of q and of k, then the rotation of the whole head.  Everything is float64 numpy on
values of T; results are 16-bit patterns.

The caps are glue_ref's, one per stage, and each stage is compared on its own: the kernel's normalised values are
observable on their own at position 0 (cos 1, sin 0: the rotation is the identity, exactly, in fp32 and in T), so a
run over all-zero positions is checked against rms_norm_ref with RMS_CAP, and the run over the real positions against
rope_ref of those normalised values with ROPE_CAP.  Chaining the two references instead would let a one-ulp step of
the norm (allowed by RMS_CAP) grow past one ulp of a rotated value where a c and b s nearly cancel, which no cap of
glue_ref covers.
"""
import collections
import functools

import numpy as np

from tests import glue_ref as ref
from tests import mla_glue_ref as mref

EPS = 1e-6                           # Qwen3's rms_norm_eps
MAX_POS = 41                         # rows of the cos_sin table; positions reach the last one
CANARY = ref.CANARY
PAD = 8                              # padding columns of the fused [q | k | v | pad] row

# fused: q, k and v are column slices of ONE [T, (H + 2 KV) D + PAD] buffer (a fused GEMM output with a padded row),
# else three dense tensors
Case = collections.namedtuple("Case", "name D n_heads n_kv_heads T fused")
CASES = [
    Case("d64-h1-t1", 64, 1, 1, 1, False),        # one wave task with 2 of 8 head groups used
    Case("d128-h3-t5", 128, 3, 1, 5, True),       # 4 heads = one full wave task
    Case("d256-h8-t33", 256, 8, 2, 33, False),    # 2 heads per wave: 5 head tasks + 1 v task; ragged last workgroup
    Case("d128-h16-t70", 128, 16, 8, 70, True),   # 6 head tasks + 2 v tasks per token
    Case("d256-h40-t5", 256, 40, 8, 5, True),     # 48 heads = 24 wave tasks: more than one wave of head groups
    Case("d64-h40-t33", 64, 40, 8, 33, False),    # 48 heads = 6 tasks of 8
]
BY_NAME = {c.name: c for c in CASES}
SLAB_CASES = ("d128-h3-t5", "d256-h8-t33", "d128-h16-t70", "d64-h1-t1")
SPLITS = (1, 2, 5)
TABLES = ("f32", "T")
assert {c.D for c in CASES} == {64, 128, 256} and {c.T for c in CASES} == {1, 5, 33, 70}
assert {(c.n_heads, c.n_kv_heads) for c in CASES} == {(1, 1), (3, 1), (8, 2), (16, 8), (40, 8)}


def n_cols(case):
    """columns of the GEMM row [q | k | v] (the slab row; the fused buffer adds PAD)"""
    return (case.n_heads + 2 * case.n_kv_heads) * case.D


def tasks_per_token(case, slabs, append=True):
    """wave tasks per token of the launch (csrc/qk_norm.hip): 512 / D heads per task, then 64 v vectors per task"""
    hpw = 512 // case.D
    head_tasks = (case.n_heads + case.n_kv_heads + hpw - 1) // hpw
    v_tasks = (case.n_kv_heads * case.D // 8 + 63) // 64 if (slabs or append) else 0
    return head_tasks + v_tasks


def n_slots(case):
    return case.T + 3


@functools.lru_cache(maxsize=None)
def index(name):
    """(positions [T] int32: 0 and MAX_POS - 1 among them where T allows, one value repeated; slot ids [T] int32:
    distinct, 0 and n_slots - 1 among them where T allows, one -1 when T >= 2)"""
    case = BY_NAME[name]
    rng = np.random.default_rng([CASES.index(case), 0x9E1])
    pos = rng.integers(0, MAX_POS, size=case.T)
    pos[-1] = MAX_POS - 1
    if case.T >= 2:
        pos[0] = 0
    if case.T >= 4:
        pos[2] = pos[1]
    free = rng.permutation(np.arange(1, n_slots(case) - 1))
    slots = np.concatenate([[0, n_slots(case) - 1], free])[:case.T]
    slots = slots[rng.permutation(case.T)]
    if case.T >= 2:
        slots[case.T // 2] = -1
    pos, slots = pos.astype(np.int32), slots.astype(np.int32)
    pos.setflags(write=False)
    slots.setflags(write=False)
    return pos, slots


@functools.lru_cache(maxsize=None)
def table(kind, bits, D):
    """[MAX_POS, D] = [cos | sin] of p * 10^6^(-2i / D) (Qwen3's rope_theta) as the kernel is given it: fp32 ("f32")
    or T ("T"), as float64.  Row 0 is cos 1, sin 0 exactly in both."""
    inv = 1.0 / 1e6 ** (np.arange(0, D, 2, dtype=np.float64) / D)
    ang = np.arange(MAX_POS, dtype=np.float64)[:, None] * inv[None, :]
    t = np.concatenate([np.cos(ang), np.sin(ang)], axis=1)
    t = t.astype(np.float32).astype(np.float64) if kind == "f32" else ref.round_to_t(t, bits)
    assert (t[0, :D // 2] == 1.0).all() and (t[0, D // 2:] == 0.0).all()
    t.setflags(write=False)
    return t


def norm_ref(x, w, eps, *, bits):
    """x [T, heads, D], w [D]: values of T -> bits [T, heads, D] of T(T(x rs) w), rs over each head's D values"""
    x = np.asarray(x, np.float64)
    T, H, D = x.shape
    return ref.rms_norm_ref(x.reshape(T * H, D), w, eps, bits=bits)[0].reshape(T, H, D)


def rope_of(n_bits, positions, tab, interleaved, *, bits):
    """the rotation stage: bits of the normalised values [T, heads, D] -> rotated bits (rope_ref, whole head)"""
    D = n_bits.shape[-1]
    return ref.rope_ref(ref.t_bits_to_f64(n_bits, bits), positions, tab, D, interleaved, bits=bits)


def reference(q, k, qw, kw, eps, positions, tab, interleaved, *, bits):
    """q [T, H, D], k [T, KV, D], qw / kw [D]: values of T.  Returns (q bits, k bits) after norm and rotation, both
    stages in float64 with one rounding each where the kernels round (the chained reference; see the module text for
    why the device test compares each stage on its own)."""
    qn, kn = norm_ref(q, qw, eps, bits=bits), norm_ref(k, kw, eps, bits=bits)
    return (rope_of(qn, positions, tab, interleaved, bits=bits), rope_of(kn, positions, tab, interleaved, bits=bits))


@functools.lru_cache(maxsize=None)
def inputs(name, bits):
    """(q [T, H, D], k [T, KV, D], v [T, KV, D], qw [D], kw [D]) as values of T.  Token 0's q and k are scaled by 32
    and, where there is one, token 1's by 2^-9 (mean of squares ~ 4e-6 against eps = 1e-6), so the statistic is not ~1
    everywhere; one head of token 0 is all zeros (rs = 1 / sqrt(eps), every output 0)."""
    case = BY_NAME[name]
    rng = np.random.default_rng([CASES.index(case), ref.BITS.index(bits), 0x9E2])
    q = rng.standard_normal((case.T, case.n_heads, case.D))
    k = rng.standard_normal((case.T, case.n_kv_heads, case.D))
    v = rng.standard_normal((case.T, case.n_kv_heads, case.D))
    for a in (q, k):
        a[0] *= 32.0
        if case.T > 1:
            a[1] *= 2.0 ** -9
    q[0, -1] = 0.0
    q, k, v = (ref.round_to_t(a, bits) for a in (q, k, v))
    qw = ref.round_to_t(1.0 + 0.25 * rng.standard_normal(case.D), bits)
    kw = ref.round_to_t(1.0 + 0.25 * rng.standard_normal(case.D), bits)
    out = (q, k, v, qw, kw)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_norm(name, bits):
    """(q bits, k bits) of the norm stage alone"""
    q, k, _, qw, kw = inputs(name, bits)
    return norm_ref(q, qw, EPS, bits=bits), norm_ref(k, kw, EPS, bits=bits)


# ---- split-K slabs ------------------------------------------------------------------------------------------------
splitk_sum_f32 = mref.splitk_sum_f32


def exact_slabs(name, n_splits):
    """fp32 [n_splits, T, N]: integers in [-3, 3] times one power of two per COLUMN ELEMENT (2^-2 .. 2^2), so the sum
    over the slices is at most 15 times that power: exact in fp32, bf16 and f16 in any order of addition"""
    case = BY_NAME[name]
    rng = np.random.default_rng([CASES.index(case), n_splits, 0x9E3])
    ints = rng.integers(-3, 4, size=(n_splits, case.T, n_cols(case)))
    scale = 2.0 ** rng.integers(-2, 3, size=(1, case.T, n_cols(case)))
    slabs = (ints * scale).astype(np.float32)
    total = slabs.astype(np.float64).sum(axis=0)
    for bits in ref.BITS:
        assert np.array_equal(ref.round_to_t(total, bits), total)
    return slabs, total


def random_slabs(name, n_splits):
    case = BY_NAME[name]
    rng = np.random.default_rng([CASES.index(case), n_splits, 0x9E4])
    return (rng.standard_normal((n_splits, case.T, n_cols(case))) / np.sqrt(n_splits)).astype(np.float32)


def split_row(case, row):
    """[T, N] -> (q [T, H, D], k [T, KV, D], v [T, KV, D]) by section 19's row layout [q | k | v]"""
    qc, kc = case.n_heads * case.D, case.n_kv_heads * case.D
    return (row[:, :qc].reshape(case.T, case.n_heads, case.D), row[:, qc:qc + kc].reshape(case.T, -1, case.D),
            row[:, qc + kc:qc + 2 * kc].reshape(case.T, -1, case.D))
