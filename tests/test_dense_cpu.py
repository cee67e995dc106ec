"""CPU tests of the dense linear boundary (include/slm_hip.h section 13): exported symbols, the ctypes mirrors of
the structs, argument validation before any launch, the plan's invariants, the exact test's case table against the
plan, and the Python layer classes' loading / sharding."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from scalellm_amd import _lib, kernels
from scalellm_amd._lib import LinearArgs, LinearPlanInfo

from . import dense_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
DEFER, SILU = _lib.SLM_LINEAR_DEFER_REDUCE, _lib.SLM_LINEAR_SILU_MUL

SYMBOLS = ["slm_linear", "slm_linear_deferred_splits", "slm_linear_plan", "slm_linear_workspace_bytes"]


@pytest.fixture(autouse=True)
def _no_knobs():
    assert _lib.lib().slm_tuning_clear(None) == 0
    yield
    assert _lib.lib().slm_tuning_clear(None) == 0


def test_the_four_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"SLM_API\s+[\w\s\*]+?\b(slm_linear\w*)\s*\(", src)))
    assert declared == SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r"\sT\s+(slm_linear\w*)", out))
    assert exported == set(SYMBOLS)
    L = _lib.lib()
    for n in SYMBOLS:
        assert getattr(L, n).argtypes is not None, n        # resolved by _lib with a prototype


@pytest.mark.parametrize("cname,cls", [("slm_linear_args", LinearArgs), ("slm_linear_plan_info", LinearPlanInfo)])
def test_linear_structs_match_the_c_header(tmp_path, cname, cls):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             f'  printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("DEFER %d\\n", SLM_LINEAR_DEFER_REDUCE);', '  printf("SILU %d\\n", SLM_LINEAR_SILU_MUL);',
              '  printf("CHIP %d\\n", SLM_LINEAR_SHARES_CHIP);', '  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out.pop("size")) == C.sizeof(cls)
    assert (int(out.pop("DEFER")), int(out.pop("SILU")), int(out.pop("CHIP"))) == \
        (DEFER, SILU, _lib.SLM_LINEAR_SHARES_CHIP)
    for fname, _ in cls._fields_:
        assert int(out[fname]) == getattr(cls, fname).offset, fname


def test_validation_precedes_any_launch():
    """host address 4096 stands for every pointer: no call may reach a kernel"""
    L = _lib.lib()
    F = lambda g: L.slm_linear(C.byref(g), None)  # noqa: E731
    A = ref.host_args
    assert L.slm_linear(None, None) == INVALID
    assert F(A(8, 4096 + 16, 4096)) == UNSUPPORTED                     # K % 32
    assert F(A(8, 4096, 4096 + 16)) == UNSUPPORTED                     # N % 32
    assert F(A(8, 4096, 4096 + 32, flags=SILU)) == UNSUPPORTED         # N % 64 with SiLU
    assert F(A(8, 4096, 4096, dtype=_lib.SLM_F32)) == UNSUPPORTED      # fp32 is no activation dtype
    assert F(A(8, 4096, 4096, lda=4088)) == INVALID                    # lda < K
    assert F(A(8, 4096, 4096, ldw=4088)) == INVALID                    # ldw < K
    assert F(A(8, 4096, 4096, ldc=4088)) == INVALID                    # ldc < N
    assert F(A(8, 4096, 4096, flags=SILU, ldc=1024)) == INVALID        # ldc < N / 2
    assert F(A(8, 4096, 4096, flags=SILU | DEFER)) == INVALID          # cannot be combined
    assert F(A(8, 4096, 4096, flags=64)) == INVALID                    # unknown flag bit
    assert F(A(8, 4096, 4096, a=None)) == INVALID
    assert F(A(8, 4096, 4096, w=None)) == INVALID
    assert F(A(8, 4096, 4096, c=None)) == INVALID
    assert F(A(-1, 4096, 4096)) == INVALID
    g = A(8, 4096, 4096)                                               # a split plan ...
    rc, info = ref.host_plan(g)
    assert rc == 0 and info.split_k > 1
    assert F(g) == WORKSPACE                                           # ... without a workspace
    g.workspace, g.workspace_bytes = 4096, info.workspace_bytes - 1
    assert F(g) == WORKSPACE                                           # ... or with too small a one
    assert F(A(0, 4096, 4096)) == 0                                    # M == 0: a no-op
    assert F(A(0, 4096, 4096, a=None, c=None)) == 0
    assert L.slm_linear_plan(C.byref(g), None) == INVALID
    assert L.slm_linear_workspace_bytes(C.byref(A(8, 4100, 4096))) == 0
    assert L.slm_linear_deferred_splits(C.byref(A(8, 4100, 4096, flags=DEFER))) == 0


PLAN_M = (1, 4, 32, 33, 64, 65, 128, 129, 300)
PLAN_KN = ((4096, 4096), (4096, 6144), (4096, 28672), (14336, 4096), (8192, 1024), (256, 32), (160, 96))


def _check_plan(M, K, N, flags, bias, info):
    L = _lib.lib()
    g = ref.host_args(M, K, N, flags=flags, bias=bias)
    s = info.split_k
    assert 1 <= s <= 16
    assert info.row_tiles in (1, 2, 4) and info.waves in (1, 2, 4) and info.waves >= info.row_tiles
    assert info.row_blocks == -(-M // (32 * info.row_tiles))
    assert info.n_chunks == K // 128 and info.tail_units == (K % 128) // 32
    # the slices tile all chunks exactly once, in order
    bounds = list(info.slice_chunk[:s + 1])
    assert bounds[0] == 0 and bounds[-1] == info.n_chunks and all(b1 >= b0 for b0, b1 in zip(bounds, bounds[1:]))
    ks = [info.slice_k_range(j) for j in range(s)]
    assert ks[0][0] == 0 and ks[-1][1] == K and all(a[1] == b[0] for a, b in zip(ks, ks[1:]))
    if s > 1:
        assert all(b1 - b0 >= 4 for b0, b1 in zip(bounds, bounds[1:])), "every slice keeps >= 4 chunks"
        assert info.row_blocks * info.col_groups * s <= 256
    if flags & SILU:
        assert s == 1 and info.waves >= 2
    assert info.workspace_bytes == (s * M * N * 4 if s > 1 else 0)
    assert L.slm_linear_workspace_bytes(C.byref(g)) == info.workspace_bytes
    want_deferred = s if (flags & DEFER) and not bias and s >= 2 else 0
    assert L.slm_linear_deferred_splits(C.byref(g)) == want_deferred


@pytest.mark.parametrize("K,N", PLAN_KN)
def test_plan_invariants(K, N):
    for M in PLAN_M:
        for flags in (0, DEFER, SILU):
            if flags & SILU and N % 64:
                continue
            for bias in (False, True):
                g = ref.host_args(M, K, N, flags=flags, bias=bias)
                rc, info = ref.host_plan(g)
                assert rc == 0, (M, K, N, flags)
                _check_plan(M, K, N, flags, bias, info)
                rc2, again = ref.host_plan(g)                          # the same args: the same plan
                assert rc2 == 0 and bytes(again) == bytes(info)


def test_the_decode_shapes_the_k_split_exists_for_are_split():
    for K, N in ((4096, 4096), (14336, 4096)):                         # o and down of Llama-3-8B
        for M in (1, 32):
            _, info = ref.host_plan(ref.host_args(M, K, N))
            assert info.split_k > 1 and info.row_blocks * info.col_groups * info.split_k == 256, (M, K, N)
    _, info = ref.host_plan(ref.host_args(32, 4096, 28672))            # gate_up fills the chip unsplit
    assert info.split_k == 1


def test_each_knob_changes_the_plan_and_clear_restores_it():
    L = _lib.lib()
    g = ref.host_args(32, 4096, 4096)
    _, base = ref.host_plan(g)
    for name, val, field in (("SLM_LINEAR_SPLITK", 3, "split_k"), ("SLM_LINEAR_RT", 2, "row_tiles"),
                             ("SLM_LINEAR_NW", 1 if base.waves != 1 else 2, "waves")):
        assert L.slm_tuning_set(name.encode(), val) == 0
        _, forced = ref.host_plan(g)
        assert getattr(forced, field) == val != getattr(base, field), name
        assert L.slm_tuning_clear(name.encode()) == 0
        _, back = ref.host_plan(g)
        assert bytes(back) == bytes(base), name
    # a forced split is capped by the chunks there are; SiLU never splits; waves never fall below the row tiles
    with kernels.tuning(SLM_LINEAR_SPLITK=5):
        assert ref.host_plan(ref.host_args(8, 256, 64))[1].split_k == 2
        assert ref.host_plan(ref.host_args(8, 96, 64))[1].split_k == 1
        assert ref.host_plan(ref.host_args(8, 4096, 128, flags=SILU))[1].split_k == 1
    with kernels.tuning(SLM_LINEAR_RT=4, SLM_LINEAR_NW=1):
        assert ref.host_plan(ref.host_args(8, 256, 64))[1].waves == 4


def test_the_exact_case_table_reaches_every_form():
    """tests/test_dense_exact_gpu.py runs EXACT_CASES: per kernel form every value of every axis and every split,
    and the plan really answers the form a row asks for"""
    seen = set()
    per_form = {f: dict(M=set(), N=set(), K=set()) for f in ref.FORMS}
    for M, N, K, rt, nw, split, bias in ref.EXACT_CASES:
        assert K <= 1312                                               # the exactness argument of int_inputs
        with kernels.tuning(**ref.knobs(rt, nw, split)):
            rc, info = ref.host_plan(ref.host_args(M, K, N, bias=bias))
        assert rc == 0
        assert (info.row_tiles, info.waves, info.split_k) == (rt, nw, split), (M, N, K)
        seen.add((rt, nw, split))
        for ax, v in (("M", M), ("N", N), ("K", K)):
            per_form[(rt, nw)][ax].add(v)
    assert seen == {(rt, nw, s) for rt, nw in ref.FORMS for s in ref.SPLITS}
    for f, axes in per_form.items():
        assert axes["M"] == set(ref.AX_M) and axes["N"] == set(ref.AX_N) and axes["K"] == set(ref.AX_K), f


# ---- the Python layer classes exist on the CPU ---------------------------------------------------------------------
def _pa(rank=0, world=1):
    from scalellm_amd.model_parallel import ParallelArgs
    return ParallelArgs(rank=rank, world_size=world)


def test_fused_loads_arrive_in_any_order_from_two_dicts():
    from scalellm_amd.layers import ColumnParallelLinear
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(n, 64, generator=g).to(torch.bfloat16) for n in (64, 32, 32))
    bq, bk, bv = (torch.randn(n, generator=g).to(torch.bfloat16) for n in (64, 32, 32))
    lin = ColumnParallelLinear(64, 128, True, False, _pa(), torch.bfloat16, "cpu")
    prefixes = ["q_proj.", "k_proj.", "v_proj."]
    with pytest.raises(RuntimeError, match="not loaded"):
        lin.verify_loaded_weights("qkv.")
    lin.load_state_dict({"v_proj.weight": v, "q_proj.bias": bq, "k_proj.weight": k}, prefixes)   # file 1
    with pytest.raises(RuntimeError, match="not loaded"):
        lin.verify_loaded_weights()
    with pytest.raises(RuntimeError, match="loaded twice"):
        lin.load_state_dict({"k_proj.weight": k}, prefixes)
    lin.load_state_dict({"q_proj.weight": q, "v_proj.bias": bv, "k_proj.bias": bk, "other.weight": q}, prefixes)
    lin.verify_loaded_weights()
    assert torch.equal(lin.weight, torch.cat([q, k, v])) and torch.equal(lin.bias, torch.cat([bq, bk, bv]))
    with pytest.raises(RuntimeError, match="loaded twice"):
        lin.load_state_dict({"q_proj.weight": q}, prefixes)


def test_plain_loads_shard_like_the_reference():
    from scalellm_amd.layers import ColumnParallelLinear, RowParallelLinear
    g = torch.Generator().manual_seed(1)
    w = torch.randn(128, 64, generator=g).to(torch.float16)
    b = torch.randn(128, generator=g).to(torch.float16)
    for rank in (0, 1):
        col = ColumnParallelLinear(64, 128, True, False, _pa(rank, 2), torch.float16, "cpu")
        col.load_state_dict({"weight": w})
        with pytest.raises(RuntimeError, match="bias is not loaded"):
            col.verify_loaded_weights()
        col.load_state_dict({"bias": b, "unrelated": w})
        col.verify_loaded_weights()
        assert torch.equal(col.weight, w[rank * 64:(rank + 1) * 64]) and col.weight.is_contiguous()   # rows: dim 0
        assert torch.equal(col.bias, b[rank * 64:(rank + 1) * 64])
        with pytest.raises(RuntimeError, match="loaded twice"):
            col.load_state_dict({"weight": w})
        row = RowParallelLinear(64, 128, True, True, _pa(rank, 2), torch.float16, "cpu")
        row.load_state_dict({"weight": w, "bias": b})
        row.verify_loaded_weights()
        assert torch.equal(row.weight, w[:, rank * 32:(rank + 1) * 32]) and row.weight.is_contiguous()  # columns: dim 1
        assert torch.equal(row.bias, b)                                                                 # whole
        with pytest.raises(ValueError):
            row.load_state_dict({"weight": w}, ["a.", "b."])            # never fused
    # the fused load shards every prefix on dim 0 before the concatenation
    gate, up = w[:64], w[64:]
    col = ColumnParallelLinear(64, 128, False, False, _pa(1, 2), torch.float16, "cpu", act_mul="silu")
    col.load_state_dict({"up_proj.weight": up}, ["gate_proj.", "up_proj."])
    col.load_state_dict({"gate_proj.weight": gate}, ["gate_proj.", "up_proj."])
    assert torch.equal(col.weight, torch.cat([gate[32:], up[32:]])) and col.paired
    with pytest.raises(ValueError):
        ColumnParallelLinear(64, 128, False, True, _pa(), torch.float16, "cpu", act_mul="silu")
    with pytest.raises(ValueError):
        ColumnParallelLinear(64, 128, False, False, _pa(), torch.float16, "cpu").load_state_dict(
            {"weight": w[:, :32]})                                      # wrong shape
    with pytest.raises(Exception):
        ColumnParallelLinear(64, 128, False, False, _pa(), torch.float32, "cpu")
    lin = ColumnParallelLinear(64, 128, False, False, _pa(), torch.float16, "cpu")
    lin.load_state_dict({"weight": w})
    with pytest.raises(kernels.SlmError):                               # no CPU fallback
        lin.forward(torch.zeros(2, 64, dtype=torch.float16))
    assert lin.deferred_splits == 0 and not lin.deferred and lin._repack() is None


def test_a_dense_step_counts_two_bytes_per_weight():
    from scalellm_amd.decode import LlamaShape, lane_query
    s = LlamaShape.llama3_8b()
    q4 = lane_query(s, 32, 8, 1, -1, 128, 128, 1, 4096)
    q16 = lane_query(s, 32, 8, 1, -1, 128, 128, 1, 4096, weight_bits=16)
    elems = 4096 * 6144 + 4096 * 4096 + 3 * 4096 * 14336
    assert q4.layer_weight_bytes == elems // 2 and q16.layer_weight_bytes == 2 * elems
    assert np.int64(q16.layer_weight_bytes) == 4 * q4.layer_weight_bytes
