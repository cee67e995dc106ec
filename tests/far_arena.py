"""Far-offset helpers: an arena that puts cache rows more than 2 GiB and more than 4 GiB from the base pointer a kernel
is given, the rule that places a case's rows there, and a sparse host model of what the arena holds.  Imports no GPU
code at module level (torch is imported inside the functions that touch the device).

The arena is ONE 1-D 16-bit tensor (torch.empty, int16 storage, viewed as bf16 / f16 by the tests):

    [ front pad 4 GiB ][ region K: 4 GiB + 64 MiB ][ region V: 4 GiB + 64 MiB ][ tail 2 MiB ]

filled with the bits of POISON_V = 256.0 (attn_exact_cases.py: finite, so that 0 * poison inside an MFMA stays 0) at
the start of every test.  A cache is a view that starts at a region's base.  A kernel that takes a byte or element
offset modulo 2^32 or 2^31, or sign-extends a 32-bit one (down to -4 GiB), lands in mapped poison -- the pad in front
of region K, region K in front of region V; the tail is there for a read past the last row of region V, which unit 0
of every placement is -- never outside the allocation: a wrong kernel gives a wrong answer, not a
fault.  Regions are never materialised on the host; rows go in and out through slices (view[s:s + n].copy_(...)), so
nothing here depends on torch's own large-index kernels.

Placement (place()): unit i of a case (a block of slots, or one row; `unit` bytes, a power of two) goes to zone (5 - i) % 6
with the in-window index i, which no other unit of the case shares:

    0  low          ALIAS + i unit                 above the alias zone [0, 32 MiB), which stays poison
    1  below 2^31   2^31 - (i + 1) unit
    2  above 2^31   2^31 + i unit
    3  below 2^32   2^32 - (i + 1) unit
    4  above 2^32   2^32 + i unit
    5  region end   REGION - (i + 1) unit          unit 0: the last rows of the view

With n unit <= WINDOW = 16 MiB every alias of an owned byte -- offset mod 2^32, offset mod 2^31, and the signed
reading of offset mod 2^32 (for region V that is region K at offset + 64 MiB) -- is poison: zones 2 and 4 alias into
[0, 16 MiB), zone 5 into (48 MiB, 64 MiB], zone 3 into zone 1's window at an index zone 1 does not use, region V's
zone 3 into region K's zone 5 window likewise, and zone 0 stays inside [32 MiB, 48 MiB).  check_placement() asserts
exactly that on the byte intervals, for one cache or for a K / V pair; tests/test_far_offsets_cpu.py runs it on every
case table of the far tests.
"""
import numpy as np

from tests import attn_exact_cases as X

MIB, GIB = 1 << 20, 1 << 30
PAD = 4 * GIB
REGION = 4 * GIB + 64 * MIB
TAIL = 2 * MIB
ARENA_BYTES = PAD + 2 * REGION + TAIL
ALIAS = 32 * MIB
WINDOW = 16 * MIB
K_BASE, V_BASE = PAD, PAD + REGION                       # byte offsets of the regions inside the arena
POISON_BITS = {"bf16": 0x4380, "f16": 0x5C00}            # 256.0
ZONES = ("low", "below 2^31", "above 2^31", "below 2^32", "above 2^32", "region end")
M31, M32 = 1 << 31, 1 << 32

assert X.POISON_V == 256.0


# ---- placement ----------------------------------------------------------------------------------------------------
def place(n, unit):
    """byte offsets (from the region's base) of n units of `unit` bytes: unit i in zone (5 - i) % 6 at in-window index i"""
    assert unit > 0 and unit & (unit - 1) == 0, ("a unit is a power of two of bytes", unit)
    assert n * unit <= WINDOW, ("the units of a case fit one window", n, unit)
    i = np.arange(n, dtype=np.int64)
    z = (5 - i) % 6
    off = np.select([z == 0, z == 1, z == 2, z == 3, z == 4],
                    [ALIAS + i * unit, M31 - (i + 1) * unit, M31 + i * unit, M32 - (i + 1) * unit, M32 + i * unit],
                    REGION - (i + 1) * unit)
    return off.astype(np.int64)


def zone_of(off, unit):
    """index into ZONES of an owned byte offset"""
    if off >= M32 + WINDOW:
        return 5
    return 4 if off >= M32 else 3 if off >= M32 - WINDOW else 2 if off >= M31 else 1 if off >= M31 - WINDOW else 0


def address_aliases(o):
    """what a kernel that mangles byte offset o reads instead: (o mod 2^32, o mod 2^31, int32 sign wrap)"""
    lo = o % M32
    return lo, o % M31, lo - M32 if lo >= M31 else lo


def check_placement(owned):
    """owned: list of (region base in the arena, byte offset from that base, length) of everything a case owns, all
    caches together.  No alias of an owned byte, taken relative to its own cache's base, may be owned by anybody."""
    iv = np.array(sorted((base + off, base + off + n) for base, off, n in owned), dtype=np.int64)
    assert len(iv) and (iv[:, 0] >= PAD).all() and (iv[:, 1] <= ARENA_BYTES - TAIL).all()
    assert (iv[1:, 0] >= iv[:-1, 1]).all(), "owned intervals overlap"
    for base, off, n in owned:
        assert 0 <= off and off + n <= REGION
        # an interval lies on one side of every multiple of 2^31: its aliases are intervals too
        assert off // M31 == (off + n - 1) // M31, (off, n)
        for a in address_aliases(off):
            if a == off:
                continue
            lo, hi = base + a, base + a + n
            assert lo >= 0, "an alias in front of the allocation"
            hit = (iv[:, 0] < hi) & (iv[:, 1] > lo)
            assert not hit.any(), (hex(off), hex(a), "an alias of an owned byte is owned", iv[hit][0].tolist())


def zones_hit(offsets, unit):
    return {zone_of(int(o), unit) for o in offsets}


# ---- sparse host model ----------------------------------------------------------------------------------------------
class Sparse:
    """slot -> row of one cache view (rows of `width` float32 values, `row_bytes` bytes each on the device); every slot
    nobody wrote reads as the poison row."""

    def __init__(self, width, row_bytes):
        self.rows, self.width, self.row_bytes = {}, width, row_bytes
        self.poison = np.full(width, X.POISON_V, np.float32)

    def put(self, slot, rows):
        for i, r in enumerate(np.asarray(rows, np.float32).reshape(-1, self.width)):
            self.rows[int(slot) + i] = r

    def get(self, slots, mangle=None):
        """rows of `slots`; mangle: what becomes of the byte offset on the way (an address mutant)"""
        out = np.empty((len(slots), self.width), np.float32)
        for i, s in enumerate(slots):
            o = int(s) * self.row_bytes
            if mangle is not None:
                o = mangle(o)
            assert o % self.row_bytes == 0
            out[i] = self.rows.get(o // self.row_bytes, self.poison)
        return out

    def owned(self, base):
        return [(base, s * self.row_bytes, self.row_bytes) for s in self.rows]


MANGLE = {"offset mod 2^32": lambda o: address_aliases(o)[0],
          "offset mod 2^31": lambda o: address_aliases(o)[1],
          "int32 sign wrap": lambda o: address_aliases(o)[2]}


# ---- far attention cases ------------------------------------------------------------------------------------------
MHA_NAMES = ["lpr_d64_g2", "w1_g4", "w2_g1", "wide_load_w2", "splits3", "bal_b20_blk16", "window10", "softcap50_d256",
             "pfdef_plain", "pf5_plain", "pf4_plain", "pf2_plain", "pf0_plain", "pfdef_d64", "kv2_1", "tile_splits2_w-1",
             "dec_tile_d128_g8", "mixed"]
MLA_NAMES = ["mla_d128_h8", "mla_d512_h24", "mla_decode_b5_s3", "mla_prefill"]
ATTN_CASES = [X.BY_NAME[n] for n in MHA_NAMES + MLA_NAMES]


class FarAttn:
    """A case of attn_exact_cases.py with its blocks moved into the far zones: block-table entry i (a whole block of
    the compact spike caches, tail included) goes to unit i of place().  Values, rounds, queries and expectations are
    the compact case's; only the slots differ.

    MHA: K and V caches [REGION / row bytes, kv heads, head_dim] at region K / region V.  MLA: the latent cache
    [.., head_dim] at region K; the RoPE-key cache [.., 64] at region V shares the slot ids, and its rows are 128 bytes:
    it reaches past 2^31 only where the latent row is 256 bytes (head_dim 128) and stays below it at head_dim 512."""

    def __init__(self, case):
        self.case, self.compact = case, X.layout(case)
        lay, B = self.compact, case.block
        mla = case.kind == "mla"
        self.k_row = (1 if mla else case.kv_heads) * case.head_dim * 2          # bytes of a slot of the K-region cache
        self.v_row = X.MLA_ROPE * 2 if mla else self.k_row
        off = place(len(lay.bt), B * self.k_row)
        self.far_bt = (off // self.k_row).astype(np.int64)
        assert self.far_bt.max() + B <= REGION // self.k_row < 2 ** 31
        self.lay = lay._replace(bt=self.far_bt.astype(np.int32), n_slots=REGION // self.k_row, owner=None, key_of=None)
        self.moves = [(int(c), int(f)) for c, f in zip(lay.bt, self.far_bt)]     # (compact slot, far slot) per block
        self._models = None

    def models(self):
        """(Sparse of the K-region cache, Sparse of the V-region cache) after the blocks were copied"""
        if self._models is None:
            self._models = self._build_models()
        return self._models

    def _build_models(self):
        K, V = X.caches(self.case, "spike")
        B, D = self.case.block, self.case.head_dim
        if self.case.kind == "mla":
            ka, va = V[:, 0], K[:, 0, D:]                    # latent, RoPE key
        else:
            ka, va = K.reshape(len(K), -1), V.reshape(len(V), -1)
        mk, mv = Sparse(ka.shape[1], self.k_row), Sparse(va.shape[1], self.v_row)
        for c, f in self.moves:
            mk.put(f, ka[c:c + B])
            mv.put(f, va[c:c + B])
        return mk, mv

    def owned(self):
        mk, mv = self.models()
        return mk.owned(K_BASE) + mv.owned(V_BASE)

    def written(self):
        """element ranges of the arena that hold the case's blocks"""
        B = self.case.block
        out = []
        for _, f in self.moves:
            out.append(((K_BASE + f * self.k_row) // 2, (K_BASE + (f + B) * self.k_row) // 2))
            out.append(((V_BASE + f * self.v_row) // 2, (V_BASE + (f + B) * self.v_row) // 2))
        return out


class FarRef(X.AttnRef):
    """AttnRef over the sparse models: the slots a sequence reads are gathered (through `mangle`, if any) into a small
    dense cache and the float64 reference runs on that."""

    def __init__(self, far, mangle=None):
        self.far, self.mangle = far, mangle
        mk, mv = far.models()
        case, lay = far.case, far.lay
        per_seq, n = [], 0
        ks, vs = [], []
        for b in range(len(lay.q_lens)):
            slots = X.AttnRef.alloc_slots(self, b, lay)
            per_seq.append(np.arange(n, n + len(slots)))
            n += len(slots)
            ks.append(mk.get(slots, mangle))
            vs.append(mv.get(slots, mangle))
        self._dense_slots = per_seq
        ka, va = np.concatenate(ks), np.concatenate(vs)
        if case.kind == "mla":
            self.K, self.V = np.concatenate([ka, va], axis=1)[:, None], ka[:, None]
        else:
            self.K, self.V = ka.reshape(n, case.kv_heads, -1), va.reshape(n, case.kv_heads, -1)

    def alloc_slots(self, b, lay):
        return self._dense_slots[b]

    def run(self, q, **kw):
        case = self.far.case
        return self(q, self.K, self.V, self.far.lay, X.sm_scale_of(case), case.softcap, case.window, X.alibi_of(case), **kw)


# ---- far rows (append and gather cases) -----------------------------------------------------------------------------
def far_rows(n, row_bytes):
    """slot ids of n rows of a cache view with `row_bytes` per slot, through all six zones"""
    off = place(n, row_bytes)
    assert len(zones_hit(off, row_bytes)) == min(n, 6)
    return (off // row_bytes).astype(np.int64)


# ---- the device side ------------------------------------------------------------------------------------------------
CHUNK = 1 << 27                                           # elements per fill / compare step (256 MiB)


def allocate():
    """the arena: int16 [ARENA_BYTES / 2] on the GPU.  A failed allocation raises."""
    import gc

    import torch
    gc.collect()                                             # an arena of the module before is dropped by now:
    torch.cuda.empty_cache()                                 # give it back first, two do not have to fit
    return torch.empty(ARENA_BYTES // 2, dtype=torch.int16, device="cuda")


def refill(arena, bits):
    for s in range(0, arena.numel(), CHUNK):
        arena[s:s + CHUNK].fill_(POISON_BITS[bits])


def view(arena, base, dtype, *shape):
    """a cache [REGION / row bytes, *shape] that starts at byte `base` of the arena"""
    row = int(np.prod(shape))
    n = REGION // (2 * row)
    return arena[base // 2:base // 2 + n * row].view(dtype).view(n, *shape)


def untouched(arena, written, bits):
    """True iff every element outside the element ranges `written` (the pad included) still holds the poison bits.
    Chunked on the device: no temporary larger than one chunk of bools."""
    import torch
    bad = torch.zeros((), dtype=torch.bool, device=arena.device)
    pos = 0
    for lo, hi in sorted(written) + [(arena.numel(), arena.numel())]:
        assert lo >= pos, "written ranges overlap"
        for s in range(pos, lo, CHUNK):
            bad |= (arena[s:min(s + CHUNK, lo)] != POISON_BITS[bits]).any()
        pos = hi
    return not bool(bad.item())


# ---- case tables of the append and gather tests ---------------------------------------------------------------------
# (name, bytes of a slot of the K-region view, bytes of a slot of the V-region view or None).  Every case uses the
# six rows of far_rows(6, K row bytes) -- one per zone -- as slot ids of BOTH views.
N_FAR = 6
APPEND = [
    ("set_kv_cache", 2 * 64 * 2, 2 * 64 * 2),                 # 2 KV heads x 64
    ("mla_set_kv_cache", 128 * 2, 64 * 2),                    # latent 128 | rope 64: the rope view moves half as far
    ("rope_kv_append vector", 2 * 64 * 2, 2 * 64 * 2),        # glue_ref.ROPE V1's shape
    ("rope_kv_append scalar", 2 * 64 * 2, 2 * 64 * 2),        # S3's shape: token stride % 4 = 2
    ("rope_kv_append slabs", 2 * 64 * 2, 2 * 64 * 2),
    ("qk_norm_rope_kv_append", 1 * 64 * 2, 1 * 64 * 2),       # qk_norm_ref d64-h1's shape
    ("qk_norm_rope_kv_append slabs", 1 * 64 * 2, 1 * 64 * 2),
    ("mla_rope_append", 128 * 2, 64 * 2),                     # mla_glue_ref h1's shape
    ("mla_rope_append slabs", 128 * 2, 64 * 2),
]
GATHER = [
    ("gemma_embed_norm", 2048 * 2, None),
    ("permute_rows", 4096 * 2, None),
    ("unpermute_rows", 4096 * 2, None),
]
ROW_CASES = {name: (k_row, v_row) for name, k_row, v_row in APPEND + GATHER}


def case_rows(name):
    """(slot ids [N_FAR], owned intervals for check_placement) of an append or gather case"""
    k_row, v_row = ROW_CASES[name]
    slots = far_rows(N_FAR, k_row)
    owned = [(K_BASE, int(s) * k_row, k_row) for s in slots]
    if v_row is not None:
        owned += [(V_BASE, int(s) * v_row, v_row) for s in slots]
    return slots, owned


def rows_written(name):
    """element ranges of the arena that an append case writes"""
    k_row, v_row = ROW_CASES[name]
    slots, _ = case_rows(name)
    out = [((K_BASE + int(s) * k_row) // 2, (K_BASE + (int(s) + 1) * k_row) // 2) for s in slots]
    if v_row is not None:
        out += [((V_BASE + int(s) * v_row) // 2, (V_BASE + (int(s) + 1) * v_row) // 2) for s in slots]
    return out


# ---- far operands of the GEMMs: reached by the row stride, the data stays tiny --------------------------------------
# the shape of tests/test_far_gemm_gpu.py's linears and what its far operands are: (rows, bytes of a row, element size)
GEMM_M, GEMM_N, GEMM_K = 33, 96, 672
GEMM_OPERANDS = {
    "A": (GEMM_M, GEMM_K * 2, 2), "C": (GEMM_M, GEMM_N * 2, 2),
    "W dense": (GEMM_N, GEMM_K * 2, 2), "W fp8": (GEMM_N, GEMM_K, 1),
    "W mxfp4": (GEMM_N, GEMM_K // 2, 1), "scales mxfp4": (GEMM_N, GEMM_K // 32, 1),
}
# the grouped MoE GEMMs: MOE_E experts [MOE_N, GEMM_K] (with their scale stacks) behind an expert stride, MOE_T rows of
# A and C.  (rows, bytes of a row -- here: of an expert --, element size)
MOE_T, MOE_E, MOE_N = 40, 3, 128
GEMM_OPERANDS.update({
    "moe A": (MOE_T, GEMM_K * 2, 2), "moe C": (MOE_T, MOE_N * 2, 2), "moe C silu": (MOE_T, MOE_N, 2),
    "experts dense": (MOE_E, MOE_N * GEMM_K * 2, 2), "experts fp8": (MOE_E, MOE_N * GEMM_K, 1),
    "experts mxfp4": (MOE_E, MOE_N * GEMM_K // 2, 1),
    "expert scales fp8": (MOE_E, MOE_N * 4, 4), "expert scales mxfp4": (MOE_E, MOE_N * GEMM_K // 32, 1),
})


def far_ld(rows, elem_size):
    """row stride in elements (a multiple of 16) that puts the last of `rows` rows 4 GiB + 16 MiB (less a little) from the
    first: the rows in between cross 2^31 on the way"""
    return (M32 + WINDOW) // elem_size // (rows - 1) // 16 * 16


def across_stride(block_bytes, elem_size):
    """expert stride in elements (a multiple of 16 bytes), just below 2^31 bytes: expert 1 starts a quarter of a block
    in front of the 2^31 mark and expert 2 half a block in front of 2^32, so offsets inside one expert cross both.
    With a uniform stride the aliases of these experts fall into other experts (expert 2 mod 2^32 into expert 0, mod
    2^31 into expert 1), not into poison: what tells a slip there is that the experts hold different values."""
    sb = (M31 - block_bytes // 4) // 16 * 16
    assert sb < M31 < sb + block_bytes and 2 * sb < M32 < 2 * sb + block_bytes and sb % elem_size == 0
    return sb // elem_size


def strided_owned(rows, row_bytes, elem_size, base=K_BASE):
    ld = far_ld(rows, elem_size)
    return [(base, r * ld * elem_size, row_bytes) for r in range(rows)]
