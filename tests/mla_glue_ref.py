"""Float64 reference and case table of the MLA prologue (include/slm_hip.h section 18: slm_mla_rope_append and its
split-K form), shared by tests/test_mla_glue_cpu.py and tests/test_mla_glue_exact_gpu.py.

The reference is built from the references tests/glue_ref.py already holds for the two kernels the prologue must
agree with bit for bit (RMSNorm: fp32 statistic, T(T(c rs) w); RoPE: one rounding of a c -/+ b s), applied to the
column ranges section 18 names.  Everything is float64 numpy on values of T; results are 16-bit patterns.
"""
import collections
import functools

import numpy as np

from tests import glue_ref as ref

ROPE = 64
EPS = 1e-6
MAX_POS = 41                         # rows of the cos_sin table; positions reach the last one
CANARY = ref.CANARY

# fused: q and kv_a are column slices of ONE [T, n_heads (nope + rope) + latent + rope + 8] buffer (a fused GEMM
# output with a padded row), else two dense tensors
Case = collections.namedtuple("Case", "name latent nope n_heads T fused")
CASES = [
    Case("h0-t1", 128, 32, 0, 1, False),         # no query at all (q = NULL), one token: two wave tasks
    Case("h1-t5", 128, 32, 1, 5, True),          # 16 rotary units: a quarter of one wave
    Case("h3-t33", 512, 128, 3, 33, False),      # latent fills the wave (64 vectors); 33 tokens x 2 tasks: a ragged
                                                 # last workgroup
    Case("h16-t70", 512, 128, 16, 70, True),     # V2-Lite's geometry: 136 units = 3 rotary tasks per token
    Case("h16-t1", 128, 128, 16, 1, True),       # decode batch 1: one workgroup
    Case("h3-t5", 512, 32, 3, 5, False),
    Case("h16-l256", 256, 32, 16, 5, True),      # the middle latent width
]
BY_NAME = {c.name: c for c in CASES}
SLAB_CASES = ("h1-t5", "h16-t70", "h3-t5", "h0-t1")
SPLITS = (1, 2, 5)
assert {c.latent for c in CASES} >= {128, 512} and {c.nope for c in CASES} == {32, 128}
assert {c.n_heads for c in CASES} == {0, 1, 3, 16} and {c.T for c in CASES} == {1, 5, 33, 70}


def n_cols(case):
    return case.n_heads * (case.nope + ROPE) + case.latent + ROPE


def tasks_per_token(case, slabs):
    """wave tasks per token of the launch (csrc/mla_glue.hip): the latent row, then 64 units per task"""
    units = (case.n_heads + 1) * (ROPE // 8) + (case.n_heads * (case.nope // 8) if slabs else 0)
    return 1 + (units + 63) // 64


def n_slots(case):
    return case.T + 3


def index(name):
    """(positions [T] int32: 0 and MAX_POS - 1 among them where T allows, one value repeated; slot ids [T] int32:
    distinct, 0 and n_slots - 1 among them where T allows, one -1 when T >= 2)"""
    case = BY_NAME[name]
    rng = np.random.default_rng([CASES.index(case), 0x31A])
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
    return pos.astype(np.int32), slots.astype(np.int32)


def table(kind, bits):
    """[MAX_POS, 64] = [cos | sin] as the kernel is given it: fp32 ("f32") or T ("T"), as float64"""
    inv = 1.0 / 10000.0 ** (np.arange(0, ROPE, 2, dtype=np.float64) / ROPE)
    ang = np.arange(MAX_POS, dtype=np.float64)[:, None] * inv[None, :]
    t = np.concatenate([np.cos(ang), np.sin(ang)], axis=1)
    return t.astype(np.float32).astype(np.float64) if kind == "f32" else ref.round_to_t(t, bits)


def reference(q, kv_a, w, eps, positions, tab, interleaved, latent, *, bits):
    """q [T, H, nope + 64] or None, kv_a [T, latent + 64], w [latent]: values of T.  Returns (latent-row bits
    [T, latent], rotated-key bits [T, 64], q bits [T, H, nope + 64] or None): what section 18 owes for every token;
    which of the first two reach a cache is the slot ids' business."""
    kv_a = np.asarray(kv_a, np.float64)
    n_bits, _ = ref.rms_norm_ref(kv_a[:, :latent], w, eps, bits=bits)
    k_bits = ref.rope_ref(kv_a[:, None, latent:latent + ROPE], positions, tab, ROPE, interleaved, bits=bits)[:, 0]
    q_bits = None
    if q is not None:
        q = np.asarray(q, np.float64)
        nope = q.shape[2] - ROPE
        q_bits = ref.f64_to_t_bits(q, bits)
        q_bits[:, :, nope:] = ref.rope_ref(q[:, :, nope:], positions, tab, ROPE, interleaved, bits=bits)
    return n_bits, k_bits, q_bits


@functools.lru_cache(maxsize=None)
def inputs(name, bits):
    """(q [T, H, nope + 64] or None, kv_a [T, latent + 64], w [latent]) as values of T.  Token 0's latent is scaled
    by 32 and, where there is one, token 1's by 2^-9 (eps-dominated), so the statistic is not ~1 everywhere."""
    case = BY_NAME[name]
    rng = np.random.default_rng([CASES.index(case), ref.BITS.index(bits), 0x31B])
    kv_a = rng.standard_normal((case.T, case.latent + ROPE))
    kv_a[0, :case.latent] *= 32.0
    if case.T > 1:
        kv_a[1, :case.latent] *= 2.0 ** -9
    kv_a = ref.round_to_t(kv_a, bits)
    w = ref.round_to_t(1.0 + 0.25 * rng.standard_normal(case.latent), bits)
    q = ref.round_to_t(rng.standard_normal((case.T, case.n_heads, case.nope + ROPE)), bits) if case.n_heads else None
    for a in (q, kv_a, w):
        if a is not None:
            a.setflags(write=False)
    return q, kv_a, w


@functools.lru_cache(maxsize=None)
def expected(name, bits, interleaved, table_kind):
    case = BY_NAME[name]
    q, kv_a, w = inputs(name, bits)
    pos, _ = index(name)
    return reference(q, kv_a, w, EPS, pos, table(table_kind, bits), interleaved, case.latent, bits=bits)


# ---- split-K slabs ------------------------------------------------------------------------------------------------
def splitk_sum_f32(slabs):
    """sum over axis 0 of fp32 slabs in the order of splitk_sum4 (csrc/common.h) for fewer than 8 slices:
    s = 0; s += (p[0] + p[1]); s += (p[2] + p[3]); ...; s += p[last] -- every step rounded to fp32"""
    slabs = np.asarray(slabs, np.float32)
    assert slabs.shape[0] < 8
    s = np.zeros(slabs.shape[1:], np.float32)
    k = 0
    while k + 2 <= slabs.shape[0]:
        s = (s + (slabs[k] + slabs[k + 1]).astype(np.float32)).astype(np.float32)
        k += 2
    if k < slabs.shape[0]:
        s = (s + slabs[k]).astype(np.float32)
    return s


def exact_slabs(name, n_splits):
    """fp32 [n_splits, T, N]: integers in [-3, 3] times one power of two per COLUMN ELEMENT (2^-2 .. 2^2), so the sum
    over the slices is at most 15 times that power: exact in fp32, bf16 and f16 in any order of addition"""
    case = BY_NAME[name]
    rng = np.random.default_rng([CASES.index(case), n_splits, 0x31C])
    ints = rng.integers(-3, 4, size=(n_splits, case.T, n_cols(case)))
    scale = 2.0 ** rng.integers(-2, 3, size=(1, case.T, n_cols(case)))
    slabs = (ints * scale).astype(np.float32)
    total = slabs.astype(np.float64).sum(axis=0)
    for bits in ref.BITS:
        assert np.array_equal(ref.round_to_t(total, bits), total)
    return slabs, total


def random_slabs(name, n_splits):
    case = BY_NAME[name]
    rng = np.random.default_rng([CASES.index(case), n_splits, 0x31D])
    return (rng.standard_normal((n_splits, case.T, n_cols(case))) / np.sqrt(n_splits)).astype(np.float32)


def split_row(case, row):
    """[T, N] -> (q [T, H, nope + 64] or None, kv_a [T, latent + 64]) by section 18's row layout [q | latent | k_pe]"""
    qc = case.n_heads * (case.nope + ROPE)
    q = row[:, :qc].reshape(case.T, case.n_heads, case.nope + ROPE) if case.n_heads else None
    return q, row[:, qc:]
