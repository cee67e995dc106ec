"""The int4 GEMM planner (csrc/w4_plan.hip) against its recorded table, without a GPU.

tests/golden/w4_plan_table.npz holds what the planner chose for ~290k (shape, M, group size, flags, bias,
perm, knob set) rows when tools/dump_w4_plans.py recorded it (the script's header names the commit and the
rows).  slm_w4a16_gemm_plan is a pure function of the argument block and the tuning table, so every field of
every row must come out the same: a change that moves a plan has to rewrite the table and say so.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location(  # tools/ is not a package: the recorder is loaded by path
    "dump_w4_plans", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "dump_w4_plans.py"))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)

K_GEMV, K_KS, K_SMALL, K_GENERAL, K_M128, K_WS, K_XL, K_XL_SK = range(8)


@pytest.fixture(scope="module")
def table():
    z = np.load(dump.TABLE)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def library(table):
    """out_* columns as the library answers the table's own in_* rows, computed once"""
    cols = {k: v for k, v in table.items() if k.startswith("in_")}
    return dump.query(table["knob_sets"], cols)


def test_table_is_the_documented_cross_product_in_integer_arrays(table):
    assert os.path.getsize(dump.TABLE) <= 256 * 1024
    assert all(np.issubdtype(v.dtype, np.integer) for v in table.values())
    knob_sets, cols = dump.table_inputs()
    assert np.array_equal(table["knob_sets"], knob_sets)
    for k, v in cols.items():
        assert np.array_equal(table[k], v), k
    assert sorted(table) == sorted(["knob_sets"] + list(cols) + ["out_" + k for k in dump.OUT])


@pytest.mark.parametrize("column", dump.OUT)
def test_every_row_plans_as_recorded(table, library, column):
    want, got = table["out_" + column], library["out_" + column]
    bad = np.flatnonzero(want != got)
    if bad.size:
        i = int(bad[0])
        row = {k[3:]: int(v[i]) for k, v in table.items() if k.startswith("in_")}
        knobs = {n: int(v) for n, v in zip(dump.KNOBS, table["knob_sets"][row["knob_set"]]) if v != dump.UNSET}
        pytest.fail(f"{column}: {bad.size} rows differ; first {row} knobs {knobs}: recorded {int(want[i])}, now {int(got[i])}")


def test_workspace_and_deferred_splits_follow_their_definitions(library, table):
    o = library
    assert np.array_equal(o["out_workspace_bytes"], o["out_part_bytes"] + o["out_aperm_bytes"])
    defers = ((table["in_flags"] & dump.DEFER) != 0) & (table["in_bias"] == 0) & (o["out_split_k"] > 1)
    assert np.array_equal(o["out_deferred_splits"], np.where(defers, o["out_split_k"], 0))
    assert defers.any() and (o["out_deferred_splits"] >= 2)[defers].all()
    # the act-order copy of A: M x K x 2 bytes rounded up to 256, after the partials
    aperm = np.where(table["in_perm"] != 0, (table["in_M"] * table["in_K"] * 2 + 255) // 256 * 256, 0)
    assert np.array_equal(o["out_aperm_bytes"], aperm)
    sk = o["out_kernel"] == K_XL_SK  # stream-K: one partial tile per workgroup + the ticket block, never slabs
    assert (o["out_part_bytes"][sk] == 256 * 256 * 256 * 4 + 2048).all() and (o["out_split_k"][sk] == 1).all()
    slabs = o["out_split_k"] * table["in_M"] * table["in_N"] * 4
    assert np.array_equal(o["out_part_bytes"][~sk], np.where(o["out_split_k"] > 1, slabs, 0)[~sk])
    assert (o["out_gemv_norm_supported"][o["out_kernel"] != K_GEMV] == 0).all()


def test_every_kernel_is_reachable_and_the_lean_one_only_behind_knobs(table):
    """Under default knobs the plan reaches every kernel but w4_small.hip: the K-sliced stream takes M <= 32
    first and steps aside only for SLM_W4_KS = 0 or a forced split it cannot realise -- those knob sets must
    keep it in the table."""
    kernel, knob_set = table["out_kernel"], table["in_knob_set"]
    assert (table["knob_sets"][0] == dump.UNSET).all()   # knob set 0: nothing forced
    default = np.bincount(kernel[knob_set == 0], minlength=8)
    assert default[K_SMALL] == 0 and (np.delete(default, K_SMALL) > 0).all(), default.tolist()
    col = {n: table["knob_sets"][:, i] for i, n in enumerate(dump.KNOBS)}
    ks_off = np.flatnonzero(col["SLM_W4_KS"] == 0)
    forced = np.flatnonzero((col["SLM_W4_SPLITK"] > 0) & (col["SLM_W4_KS"] == dump.UNSET))
    for sets in (ks_off, forced):
        assert (kernel[np.isin(knob_set, sets)] == K_SMALL).any()
    # one or two row tiles of the K-sliced stream, and the general kernel's three tile heights, all occur
    assert set(table["out_row_tiles"][kernel == K_KS]) == {1, 2}
    assert set(table["out_row_tiles"][kernel == K_GENERAL]) == {1, 2, 4}


def test_plan_query_rejects_what_the_gemm_rejects():
    from scalellm_amd import _lib
    L = _lib.lib()
    g, info = _lib.W4GemmArgs(), _lib.W4PlanInfo()
    g.M, g.K, g.N, g.lda, g.ldc, g.group_size, g.dtype = 8, 4096, 4096, 4096, 4096, 128, _lib.SLM_BF16
    assert L.slm_w4a16_gemm_plan(C.byref(g), C.byref(info)) == 0 and info.kernel_name == "KS"
    assert L.slm_w4a16_gemm_plan(C.byref(g), None) != 0 and L.slm_w4a16_gemm_plan(None, C.byref(info)) != 0
    for field, value in (("K", 4096 + 64), ("N", 4096 + 16), ("group_size", 48), ("flags", 8),
                         ("flags", _lib.SLM_W4_SILU_MUL | _lib.SLM_W4_DEFER_REDUCE), ("dtype", 7)):
        bad = _lib.W4GemmArgs.from_buffer_copy(g)
        setattr(bad, field, value)
        assert L.slm_w4a16_gemm_plan(C.byref(bad), C.byref(info)) != 0, (field, value)
        assert L.slm_w4a16_gemm_workspace_bytes(C.byref(bad)) == 0
