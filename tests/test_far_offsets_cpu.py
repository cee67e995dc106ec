"""The far-offset tests without a GPU: the placement of every case table of tests/test_far_*_gpu.py meets the alias
condition of tests/far_arena.py, relocation leaves the spike conditions of the attention cases intact, and a reference
that mangles the byte offset of a cache row the way a kernel with a 32-bit slip would -- offset mod 2^32, offset mod
2^31, int32 sign wrap; read through the sparse model of the arena -- breaks the assertion the GPU test makes, on
every case.  That is the evidence that the GPU tests would notice."""
import numpy as np
import pytest

from tests import attn_exact_cases as X
from tests import far_arena as F
from tests.attn_exact_cases import f64_to_t_bits, t_ulp_distance

ATTN = [pytest.param(c, id=c.name) for c in F.ATTN_CASES]


@pytest.mark.parametrize("n,unit", [(1, 128), (6, 128), (7, 4096), (4096, 4096), (64, 1 << 18)])
def test_place_zones_and_alias_condition(n, unit):
    off = F.place(n, unit)
    assert len(set(off.tolist())) == n
    assert [F.zone_of(int(o), unit) for o in off[:6]] == [5, 4, 3, 2, 1, 0][:n]
    assert off[0] + unit == F.REGION                         # the last rows of the view
    for base in (F.K_BASE, F.V_BASE):
        F.check_placement([(base, int(o), unit) for o in off])
    F.check_placement([(b, int(o), unit) for b in (F.K_BASE, F.V_BASE) for o in off])


def test_check_placement_sees_an_owned_alias():
    unit = 4096
    for bad in ([(F.K_BASE, F.M32 + unit, unit), (F.K_BASE, unit, unit)],                      # mod 2^32
                [(F.K_BASE, F.M31 + unit, unit), (F.K_BASE, unit, unit)],                      # mod 2^31
                [(F.K_BASE, F.M32 - unit, unit), (F.K_BASE, F.M31 - unit, unit)],              # mod 2^31, mark to mark
                [(F.V_BASE, F.M32 - unit, unit), (F.K_BASE, F.REGION - unit, unit)]):          # sign wrap, V into K
        with pytest.raises(AssertionError):
            F.check_placement(bad)


@pytest.mark.parametrize("case", ATTN)
def test_attention_placement(case):
    far = F.FarAttn(case)
    F.check_placement(far.owned())
    unit = case.block * far.k_row
    assert F.zones_hit([f * far.k_row for _, f in far.moves], unit) == set(range(6)), "blocks in every zone"
    # every sequence's keys are where the compact layout has them, block by block
    lay = X.layout(case)
    for b, kv in enumerate(case.kv_lens):
        j = np.arange(kv)
        c, f = X.slot_of(lay, b, j), X.slot_of(far.lay, b, j)
        moved = dict(far.moves)
        assert all(moved[int(cs - jj % case.block)] + jj % case.block == fs for cs, fs, jj in zip(c, f, j))


def _exact_rows_off(case, ref, bits="bf16", stop_at_first=True):
    """rounds in which some exact row of `ref` differs from spike_expect (the GPU test's 0-ulp assertion)"""
    n, off = sum(case.q_lens), []
    for r, rnd in enumerate(X.rounds(case)):
        out, _ = ref.run(X.spike_q(case, rnd))
        ex = rnd.exact[:n]
        d = t_ulp_distance(f64_to_t_bits(out[:n], bits), f64_to_t_bits(X.spike_expect(case, rnd)[:n], bits))
        if d[ex].any():
            off.append(r)
            if stop_at_first:
                break
    return off


@pytest.mark.parametrize("case", ATTN)
def test_far_attention_keeps_the_spike_conditions(case):
    """Relocation changes slots, not values: leak <= LEAK_CAP on every exact row of every round, and the float64
    reference over the sparse model returns V[target] bit for bit."""
    far = F.FarAttn(case)
    ref = F.FarRef(far)
    _, V = X.caches(case, "spike")
    real = np.abs(V[X.layout(case).owner >= 0])
    ratio = float(real.max() / real.min())
    assert ratio < 2.0
    n = sum(case.q_lens)
    for r, rnd in enumerate(X.rounds(case)):
        out, leak = ref.run(X.spike_q(case, rnd))
        ex = rnd.exact[:n]
        worst = float(leak[:n][ex].max()) if ex.any() else 0.0
        assert worst * ratio <= X.LEAK_CAP, (case.name, r, rnd.kind, "leak", worst)
        for bits in case.bits:
            d = t_ulp_distance(f64_to_t_bits(out[:n], bits), f64_to_t_bits(X.spike_expect(case, rnd)[:n], bits))
            assert not d[ex].any(), (case.name, r, rnd.kind, bits)


@pytest.mark.parametrize("what", list(F.MANGLE))
@pytest.mark.parametrize("case", ATTN)
def test_address_mutants_break_the_spike_expectation(case, what):
    far = F.FarAttn(case)
    assert _exact_rows_off(case, F.FarRef(far, F.MANGLE[what])), (case.name, what, "no exact row noticed")


# ---- append and gather cases: placement, and the mutants against row equality -------------------------------------
ROWS = [pytest.param(name, id=name.replace(" ", "-")) for name in F.ROW_CASES]


@pytest.mark.parametrize("name", ROWS)
def test_rows_placement(name):
    slots, owned = F.case_rows(name)
    F.check_placement(owned)
    k_row, _ = F.ROW_CASES[name]
    assert [F.zone_of(int(s) * k_row, k_row) for s in slots] == [5, 4, 3, 2, 1, 0]
    assert int(slots.max()) < 2 ** 31 and (int(slots[0]) + 1) * k_row == F.REGION


def _scatter_then_read(slots, row_bytes, mangle):
    """rows 1 .. n written to `slots` by a kernel that mangles the offset, read back at the true slots"""
    m = F.Sparse(1, row_bytes)
    for i, s in enumerate(slots):
        o = int(s) * row_bytes
        m.rows[(mangle(o) if mangle else o) // row_bytes] = np.array([i + 1.0], np.float32)
    return m.get(slots)[:, 0]


def _gather(slots, row_bytes, mangle):
    m = F.Sparse(1, row_bytes)
    for i, s in enumerate(slots):
        m.put(s, [i + 1.0])
    return m.get(slots, mangle)[:, 0]


@pytest.mark.parametrize("name", ROWS)
def test_address_mutants_break_row_equality(name):
    """the far rows equal the compact call's rows (values 1 .. n here) for the true addressing and for no mutant"""
    slots, _ = F.case_rows(name)
    want = np.arange(1.0, len(slots) + 1)
    append = name in {n for n, _, _ in F.APPEND}
    model = _scatter_then_read if append else _gather
    for row_bytes in (r for r in F.ROW_CASES[name] if r is not None):
        far_enough = int(slots.max()) * row_bytes >= F.M32        # the rope view of the MLA cases stops short of 2^32
        assert np.array_equal(model(slots, row_bytes, None), want)
        for what, mangle in F.MANGLE.items():
            broken = not np.array_equal(model(slots, row_bytes, mangle), want)
            assert broken or (what == "offset mod 2^32" and not far_enough), (name, row_bytes, what)
    k_row = F.ROW_CASES[name][0]
    for what, mangle in F.MANGLE.items():                          # the K-region view catches every one
        assert not np.array_equal(model(slots, k_row, mangle), want), (name, what)


# ---- the int4 GEMM plan steps off its 32-bit paths (host only, as test_w4_plan_cpu.py) ------------------------------
def _w4_plan(M, K, N, lda=None, ldc=None):
    import ctypes as C
    from scalellm_amd import _lib
    g, info = _lib.W4GemmArgs(), _lib.W4PlanInfo()
    g.M, g.K, g.N, g.lda, g.ldc, g.group_size, g.dtype = M, K, N, lda or K, ldc or N, 128, _lib.SLM_BF16
    assert _lib.lib().slm_w4a16_gemm_plan(C.byref(g), C.byref(info)) == 0
    return info.kernel_name, info.row_tiles


# (M, K, N): (kernel, row tiles) for compact operands, for far A and for far C (row stride far_arena.far_ld: the last
# row past 4 GiB) -- what tests/test_far_gemm_gpu.py asserts before it launches the cases it takes from here
W4_FAR_PLANS = {
    (8, 4096, 4096): (("KS", 1), ("GENERAL", 1), ("SMALL", 1)),
    (33, 4096, 4096): (("KS", 2), ("GENERAL", 2), ("GENERAL", 2)),
    (33, 1024, 512): (("KS", 2), ("GENERAL", 2), ("GENERAL", 2)),
    (64, 4096, 28672): (("KS", 2), ("GENERAL", 2), ("GENERAL", 2)),
    (129, 512, 14336): (("WS", 8), ("GENERAL", 2), ("WS", 8)),
    (129, 4096, 14336): (("WS", 8), ("GENERAL", 2), ("WS", 8)),
}


@pytest.mark.parametrize("M,K,N", list(W4_FAR_PLANS))
def test_w4_plan_leaves_the_i31_kernels_for_far_strides(M, K, N):
    """w4_plan.hip: a_fits_i31 / c_fits_i31 are false once the last row of A / C starts 2 GiB from the pointer; the
    K-sliced stream (KS) needs both, the lean kernel (SMALL) needs A, row tiles of 8 and more need A."""
    far = F.far_ld(M, 2)
    assert (M - 1) * far * 2 >= 1 << 32 and (M - 1) * max(K, N) * 2 < 1 << 31
    got = (_w4_plan(M, K, N), _w4_plan(M, K, N, lda=far), _w4_plan(M, K, N, ldc=far))
    assert got == W4_FAR_PLANS[(M, K, N)]
    near, far_a, far_c = got
    assert far_a != near and (far_c != near or near[0] == "WS")      # WS keeps no 32-bit offset into C


@pytest.mark.parametrize("what", list(F.GEMM_OPERANDS))
def test_gemm_far_strides_meet_the_alias_condition(what):
    rows, row_bytes, es = F.GEMM_OPERANDS[what]
    owned = F.strided_owned(rows, row_bytes, es)
    F.check_placement(owned)
    offs = [o for _, o, _ in owned]
    assert offs[-1] >= F.M32 and offs[-1] + row_bytes <= F.REGION and any(F.M31 <= o < F.M32 for o in offs)
    want = np.arange(1.0, rows + 1)
    for name, mangle in F.MANGLE.items():                      # a row read (or written) through a mangled offset
        m = F.Sparse(1, 1)
        for i, o in enumerate(offs):
            m.rows[o] = np.array([i + 1.0], np.float32)
        got = np.array([m.rows.get(mangle(o), m.poison)[0] for o in offs])
        assert not np.array_equal(got, want), (what, name)


@pytest.mark.parametrize("split", (0, 1, 3))
@pytest.mark.parametrize("kind", ("dense", "fp8", "mxfp4"))
def test_linear_plans_do_not_depend_on_the_strides(kind, split):
    """The dense, fp8 and mxfp4 linears address rows in 64 bits on every path: far lda / ldw (lds) / ldc change no
    field of the plan (host only; test_far_gemm_gpu.py asserts the same on the device)."""
    from scalellm_amd import kernels
    from tests import dense_ref, fp8_ref, mxfp4_ref
    mod = {"dense": dense_ref, "fp8": fp8_ref, "mxfp4": mxfp4_ref}[kind]
    fields = ("row_tiles", "waves", "row_blocks", "col_groups", "split_k", "n_chunks", "tail_units", "lds_bytes",
              "workspace_bytes")
    w_es = 2 if kind == "dense" else 1
    far = [dict(lda=F.far_ld(F.GEMM_M, 2)), dict(ldw=F.far_ld(F.GEMM_N, w_es)), dict(ldc=F.far_ld(F.GEMM_M, 2))]
    if kind == "mxfp4":
        far[1]["lds"] = F.far_ld(F.GEMM_N, 1)
    with kernels.tuning(SLM_LINEAR_SPLITK=split):
        rc, near = mod.host_plan(mod.host_args(F.GEMM_M, F.GEMM_K, F.GEMM_N))
        assert rc == 0
        for kw in far:
            rc, plan = mod.host_plan(mod.host_args(F.GEMM_M, F.GEMM_K, F.GEMM_N, **kw))
            assert rc == 0 and all(getattr(plan, f) == getattr(near, f) for f in fields), (kind, kw)
            assert list(plan.slice_chunk) == list(near.slice_chunk)


@pytest.mark.parametrize("what", [w for w in F.GEMM_OPERANDS if w.startswith("expert")])
def test_expert_strides_across_the_marks(what):
    """across_stride(): offsets inside expert 1 cross 2^31, inside expert 2 cross 2^32, everything stays inside the
    region, and each mutant moves some byte of an expert to a place that holds something else (another expert's
    bytes at another in-expert offset, or poison)."""
    n, block, es = F.GEMM_OPERANDS[what]
    sb = F.across_stride(block, es) * es
    assert n == 3 and 2 * sb + block <= F.REGION
    where = {}                                               # byte -> (expert, offset in it), at the probed bytes
    probes = [(e, o) for e in range(n) for o in (0, block // 4 - 1, block // 4, block // 2 - 1, block // 2, block - 1)]
    for e, o in probes:
        where[e * sb + o] = (e, o)
    for name, mangle in F.MANGLE.items():
        moved = [(e, o) for e, o in probes if mangle(e * sb + o) != e * sb + o]
        assert moved, (what, name)
        for e, o in moved:
            assert where.get(mangle(e * sb + o)) != (e, o)
