"""Record what the int4 GEMM planner (csrc/w4_plan.hip) chooses into tests/golden/w4_plan_table.npz.

    python tools/dump_w4_plans.py            # rewrite the table from the library as built
    python tools/dump_w4_plans.py --check    # compare the library with the committed table, write nothing

The committed table was recorded from commit e9738a8 ("Add int4 mixture-of-experts ..."), the last one with
the single 310-line plan_gemm in w4.hip, through a slm_w4a16_gemm_plan that read the kernel id off that
function's flags in gemm_impl's if / else order.  Its workspace_bytes and deferred_splits columns were also
compared against an unmodified build of that commit (both functions are in its ABI): equal on every row.
tests/test_w4_plan_cpu.py holds every later planner to it; rewrite the table only together with a change
that means to change a plan, and say so in that change.

The planner makes no HIP call, so this runs without a GPU.  Integer arrays only:
    knob_sets [S, len(KNOBS)]   one row per knob set, UNSET where a knob is left alone
    in_*      [R]               M, K, N, group_size, flags, bias, perm (0 / 1: pointer present), knob_set (row of knob_sets)
    out_*     [R]               every field of slm_w4_plan_info, then workspace_bytes, deferred_splits and
                                gemv_norm_supported as their own ABI functions answer

Rows.  Default knobs: the full cross product of SHAPES x MS x GROUPS x FLAGS x (bias, perm), less the invalid
combinations (group_size that does not divide K, SILU_MUL on N % 64 != 0).  Forced knob sets -- every combination
tests/test_w4_gpu.py, tests/test_w4_silu_gpu.py and tools/bench_small_gemm.py runs set (test_w8_gpu.py and
test_decode_lanes_gpu.py set none) -- cross the same shapes and flags with the row counts of the regime their
kernel-selecting knob acts in plus the first row count on either side of it (KNOB_M_RANGE), group sizes
32 / 64 / 128 (the plan sees a group size only as scale groups per chunk: 4 / 2 / 1) and no bias / perm: the
full product over ~130 knob sets would not fit the 256 KB the fixture may take.
"""
import argparse
import ctypes as C
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, "tests", "golden", "w4_plan_table.npz")

UNSET = -(2 ** 31)
KNOBS = ("SLM_W4_GEMV", "SLM_W4_GEMV_KS", "SLM_W4_SMALL", "SLM_W4_MT", "SLM_W4_NTW", "SLM_W4_SPLITK",
         "SLM_W4_KS", "SLM_W4_KS_CW", "SLM_W4_KS_NW", "SLM_W4_KS_TPW", "SLM_W4_KS_MT2", "SLM_W4_M128",
         "SLM_W4_M128_WD", "SLM_W4_M128_KW", "SLM_W4_M128_CT", "SLM_W4_M128_ADMA", "SLM_W4_XL_SK")

SHAPES = (  # (K, N)
    (4096, 6144), (4096, 4096), (4096, 28672), (14336, 4096),        # Llama-3-8B
    (8192, 10240), (8192, 8192), (8192, 57344), (28672, 8192),       # Llama-3-70B
    (8192, 1280), (8192, 7168), (1024, 8192), (3584, 8192),          # its TP = 8 shards
    (1152, 288), (640, 160), (1792, 224), (1024, 480), (2048, 384), (1024, 2048))  # the GPU grids' odd shapes
# (the GPU grids write those as N x K: 288 x 1152 ...; K has to be a multiple of 128)
MS = (1, 2, 4, 5, 17, 32, 33, 48, 64, 65, 96, 128, 129, 256, 512, 1536, 2048, 2304, 2648, 3072, 4000)
GROUPS = (32, 64, 128, 256, 0)  # 0 = K (per channel)
DEFER, SILU, CHIP = 1, 2, 4
FLAGS = (0, DEFER, SILU, CHIP, DEFER | CHIP)

# row counts a forced knob set is crossed with: the regime of its kernel-selecting knob (first match)
KNOB_M_RANGE = (("SLM_W4_M128", 65, 128), ("SLM_W4_XL_SK", 129, 1 << 30), ("SLM_W4_GEMV", 1, 4),
                ("SLM_W4_GEMV_KS", 1, 4), ("SLM_W4_KS_MT2", 33, 64), ("SLM_W4_KS", 1, 64),
                ("SLM_W4_KS_CW", 1, 32), ("SLM_W4_KS_NW", 1, 32), ("SLM_W4_KS_TPW", 1, 64),
                ("SLM_W4_SMALL", 1, 32))  # SLM_W4_MT / SLM_W4_NTW / SLM_W4_SPLITK alone: every row count


def _knob_sets():
    sets = [{}]

    def add(**kw):
        if kw not in sets:
            sets.append(kw)
    # tests/test_w4_gpu.py
    for mt in (8, 16):                                    # ws / xl grids, repeated launches
        add(SLM_W4_MT=mt)
        for sk in (0, 2, 7, 4):
            add(SLM_W4_MT=mt, SLM_W4_SPLITK=sk)
    for wd, kw, ct, adma in ((2, 1, 4, 0), (4, 1, 4, 0), (2, 2, 4, 0), (4, 2, 4, 0), (2, 1, 8, 0), (4, 1, 8, 0),
                             (2, 1, 8, 1), (4, 1, 8, 1)):  # m128 grid
        form = dict(SLM_W4_M128_WD=wd, SLM_W4_M128_KW=kw, SLM_W4_M128_CT=ct, SLM_W4_M128_ADMA=adma)
        add(SLM_W4_M128=1, **form)
        for sk in (0, 2, 7, 4, 3):
            add(SLM_W4_M128=1, SLM_W4_SPLITK=sk, **form)
        add(SLM_W4_M128=0, SLM_W4_SPLITK=0, **form)
    add(SLM_W4_GEMV=2)
    for kn in ({}, dict(SLM_W4_KS_TPW=3), dict(SLM_W4_KS_CW=1), dict(SLM_W4_KS_CW=2, SLM_W4_KS_NW=4),
               dict(SLM_W4_KS_CW=2), dict(SLM_W4_KS_CW=4, SLM_W4_KS_NW=4), dict(SLM_W4_KS_CW=1, SLM_W4_KS_TPW=2),
               dict(SLM_W4_KS_NW=4, SLM_W4_KS_CW=2, SLM_W4_KS_TPW=5)):
        add(SLM_W4_KS=1, **kn)
    for kn in ({}, dict(SLM_W4_KS_MT2=2), dict(SLM_W4_KS_TPW=4), dict(SLM_W4_KS_TPW=2)):
        add(**{"SLM_W4_KS_MT2": 1, **kn})
    add(SLM_W4_KS_MT2=0)
    add(SLM_W4_KS=0)
    add(SLM_W4_XL_SK=0)
    add(SLM_W4_XL_SK=2)
    # tests/test_w4_silu_gpu.py
    add(SLM_W4_GEMV_KS=4)
    add(SLM_W4_GEMV_KS=2)
    add(SLM_W4_GEMV=2, SLM_W4_GEMV_KS=4)
    add(SLM_W4_SMALL=0, SLM_W4_SPLITK=1)
    add(SLM_W4_SMALL=0, SLM_W4_SPLITK=1, SLM_W4_NTW=2)
    add(SLM_W4_KS_MT2=1, SLM_W4_KS_TPW=4)
    add(SLM_W4_KS=0, SLM_W4_SPLITK=1)
    add(SLM_W4_KS_MT2=0, SLM_W4_SPLITK=1)
    for sk in (1, 2):
        add(SLM_W4_MT=4, SLM_W4_SPLITK=sk)
    add(SLM_W4_MT=8, SLM_W4_SPLITK=1)
    add(SLM_W4_MT=16, SLM_W4_SPLITK=1)
    add(SLM_W4_M128=1)
    add(SLM_W4_M128=1, SLM_W4_SPLITK=1)
    add(SLM_W4_M128=1, SLM_W4_SPLITK=4)
    add(SLM_W4_M128=1, SLM_W4_M128_WD=4, SLM_W4_SPLITK=1)
    add(SLM_W4_M128=1, SLM_W4_M128_KW=2, SLM_W4_SPLITK=1)
    add(SLM_W4_M128=1, SLM_W4_M128_KW=2, SLM_W4_SPLITK=2)
    add(SLM_W4_M128=1, SLM_W4_M128_KW=1, SLM_W4_SPLITK=1)
    add(SLM_W4_M128=1, SLM_W4_M128_CT=8, SLM_W4_SPLITK=1)
    add(SLM_W4_M128=1, SLM_W4_M128_CT=8, SLM_W4_SPLITK=2)
    add(SLM_W4_M128=1, SLM_W4_M128_CT=8, SLM_W4_M128_WD=4)
    add(SLM_W4_M128=1, SLM_W4_M128_CT=8, SLM_W4_M128_ADMA=1, SLM_W4_SPLITK=1)
    add(SLM_W4_M128=1, SLM_W4_M128_CT=8, SLM_W4_M128_ADMA=1, SLM_W4_SPLITK=2)
    # tools/bench_small_gemm.py sweeps (and the silu grid's bare SLM_W4_SPLITK cases)
    for sk in range(1, 9):
        add(SLM_W4_SPLITK=sk)
    add(SLM_W4_SMALL=0)
    return sets


def _ms_of(knobs):
    for name, lo, hi in KNOB_M_RANGE:
        if name in knobs:
            inside = [i for i, m in enumerate(MS) if lo <= m <= hi]
            return MS[max(inside[0] - 1, 0):inside[-1] + 2]
    return MS


def table_inputs():
    """(knob_sets [S, len(KNOBS)], dict of in_* columns)"""
    sets = _knob_sets()
    knob_sets = np.full((len(sets), len(KNOBS)), UNSET, np.int64)
    rows = []
    for s, knobs in enumerate(sets):
        for name, v in knobs.items():
            knob_sets[s, KNOBS.index(name)] = v
        ms, groups = (MS, GROUPS) if not knobs else (_ms_of(knobs), (32, 64, 128))
        bps = ((0, 0), (1, 0), (0, 1), (1, 1)) if not knobs else ((0, 0),)
        for (K, N), M, gs, fl, (bias, perm) in itertools.product(SHAPES, ms, groups, FLAGS, bps):
            gs = gs or K
            if K % gs or (gs == K and K in GROUPS) or (fl & SILU and N % 64):
                continue
            rows.append((M, K, N, gs, fl, bias, perm, s))
    cols = np.array(rows, np.int64).T
    names = ("M", "K", "N", "group_size", "flags", "bias", "perm", "knob_set")
    return knob_sets, {"in_" + n: c for n, c in zip(names, cols)}


OUT = ("kernel", "row_tiles", "n_mblocks", "n_nblocks", "split_k", "chunks_per_split", "variant0", "variant1",
       "variant2", "variant3", "lds_bytes", "part_bytes", "aperm_bytes", "workspace_bytes", "deferred_splits",
       "gemv_norm_supported")


def query(knob_sets, cols, plan=True):
    """out_* columns the library as built gives the rows of `cols` (plan=False: the three older queries only)"""
    from scalellm_amd import _lib
    L = _lib.lib()
    n = len(cols["in_M"])
    out = {"out_" + k: np.zeros(n, np.int64) for k in (OUT if plan else OUT[-3:])}
    g, info, cur = _lib.W4GemmArgs(), _lib.W4PlanInfo() if plan else None, None
    g.dtype = _lib.SLM_BF16
    try:
        for i in range(n):
            s = int(cols["in_knob_set"][i])
            if s != cur:
                L.slm_tuning_clear(None)
                for name, v in zip(KNOBS, knob_sets[s]):
                    if v != UNSET:
                        assert L.slm_tuning_set(name.encode(), int(v)) == 0, name
                cur = s
            g.M, g.K, g.N = int(cols["in_M"][i]), int(cols["in_K"][i]), int(cols["in_N"][i])
            g.group_size, g.flags = int(cols["in_group_size"][i]), int(cols["in_flags"][i])
            g.lda, g.ldc = g.K, g.N // 2 if g.flags & SILU else g.N
            g.bias = 64 if cols["in_bias"][i] else None   # (pointers are only tested for NULL)
            g.perm = 64 if cols["in_perm"][i] else None
            if plan:
                rc = L.slm_w4a16_gemm_plan(C.byref(g), C.byref(info))
                assert rc == 0, (rc, g.M, g.K, g.N, g.group_size, g.flags)
                for k in OUT[:6] + OUT[10:13]:
                    out["out_" + k][i] = getattr(info, k)
                for j in range(4):
                    out["out_variant%d" % j][i] = info.variant[j]
            out["out_workspace_bytes"][i] = L.slm_w4a16_gemm_workspace_bytes(C.byref(g))
            out["out_deferred_splits"][i] = L.slm_w4a16_gemm_deferred_splits(C.byref(g))
            out["out_gemv_norm_supported"][i] = L.slm_w4a16_gemv_norm_supported(C.byref(g))
    finally:
        L.slm_tuning_clear(None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed table, write nothing")
    ap.add_argument("--abi-only", action="store_true",
                    help="with --check: only the columns older libraries answer (workspace_bytes, deferred_splits, "
                         "gemv_norm_supported) -- the independent anchor against a build without the plan query")
    args = ap.parse_args()
    knob_sets, cols = table_inputs()
    out = query(knob_sets, cols, plan=not args.abi_only)
    if args.check:
        z = np.load(TABLE)
        assert np.array_equal(z["knob_sets"], knob_sets)
        bad = [k for k in list(cols) + list(out) if not np.array_equal(z[k], {**cols, **out}[k])]
        print(f"{len(cols['in_M'])} rows, {len(out)} output columns compared:", "MISMATCH " + str(bad) if bad else "equal")
        sys.exit(1 if bad else 0)
    small = {k: v.astype(np.int32) if np.abs(v).max() < 2 ** 31 else v for k, v in {**cols, **out}.items()}
    np.savez_compressed(TABLE, knob_sets=knob_sets, **small)
    kern = out["out_kernel"]
    print(f"{TABLE}: {len(kern)} rows, {os.path.getsize(TABLE)} bytes; rows per kernel id", np.bincount(kern, minlength=8).tolist(),
          "default knobs", np.bincount(kern[cols["in_knob_set"] == 0], minlength=8).tolist())


if __name__ == "__main__":
    main()
