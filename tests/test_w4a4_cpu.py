"""CPU tests of the MXFP4 x MXFP4 linear boundary (include/slm_hip.h section 22): the symbols, the ctypes mirror of
the argument block, the plan without a GPU under the entry's own knobs, and validation before any launch."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from scalellm_amd import _lib, kernels
from scalellm_amd._lib import Mxfp4LinearArgs, W4A4LinearArgs

from . import w4a4_ref as ref

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slm_hip.h")
INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT = -1, -2, -3, -5
DEFER, SILU = _lib.SLM_LINEAR_DEFER_REDUCE, _lib.SLM_LINEAR_SILU_MUL
SYMBOLS = ["slm_w4a4_linear", "slm_w4a4_linear_deferred_splits", "slm_w4a4_linear_plan", "slm_w4a4_quantize_act"]


@pytest.fixture(autouse=True)
def _no_knobs():
    assert _lib.lib().slm_tuning_clear(None) == 0
    yield
    assert _lib.lib().slm_tuning_clear(None) == 0


def test_the_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"SLM_API\s+[\w\s\*]+?\b(slm_w4a4_\w*)\s*\(", src))) == SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r"\sT\s+(slm_w4a4_\w*)", out)) == set(SYMBOLS)
    for n in SYMBOLS:
        assert getattr(_lib.lib(), n).argtypes is not None, n
    for n in ("quantize_mxfp4_act", "w4a4_linear", "w4a4_linear_plan"):
        assert callable(getattr(kernels, n)), n


def test_the_argument_block_matches_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(slm_w4a4_linear_args));', '  printf("mx_size %zu\\n", sizeof(slm_mxfp4_linear_args));']
    for fname, _ in W4A4LinearArgs._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(slm_w4a4_linear_args, {fname}));')
    for fname, _ in Mxfp4LinearArgs._fields_:
        lines.append(f'  printf("mx_{fname} %zu\\n", offsetof(slm_mxfp4_linear_args, {fname}));')
    (tmp_path / "abi.c").write_text("\n".join(lines + ['  return 0;', '}']))
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")])
    out = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([str(tmp_path / "abi")], text=True).splitlines())}
    assert out["size"] == C.sizeof(W4A4LinearArgs)
    for fname, _ in W4A4LinearArgs._fields_:
        assert out[fname] == getattr(W4A4LinearArgs, fname).offset, fname
    for fname, _ in Mxfp4LinearArgs._fields_:                          # section 20's block, field for field, then two
        assert out[fname] == out["mx_" + fname], fname
    assert out["a_scale"] == out["mx_size"] and out["ldas"] == out["a_scale"] + 8


def test_the_plan_answers_without_a_gpu_under_its_own_knobs():
    L = _lib.lib()
    for M, N, K, rt, nw, split, bias in ref.EXACT_CASES:
        with kernels.tuning(**ref.knobs(rt, nw, split)):
            for flags in (0, DEFER):
                g = ref.host_args(M, K, N, bias=bias, flags=flags, quantised=bool(flags))
                rc, info = ref.host_plan(g)
                assert rc == 0 and (info.row_tiles, info.waves, info.split_k) == (rt, nw, split), (M, N, K)
                assert info.n_chunks == K // 128 and info.tail_units == (K % 128) // 32
                assert info.slice_k_range(0)[0] == 0 and info.slice_k_range(split - 1)[1] == K
                assert info.workspace_bytes == (split * M * N * 4 if split > 1 else 0)
                assert info.lds_bytes == 2 * 32 * rt * 68
                want = split if (flags & DEFER) and not bias and split >= 2 else 0
                assert L.slm_w4a4_linear_deferred_splits(C.byref(g)) == want
    base = ref.host_plan(ref.host_args(8, 4096, 4096))[1]
    with kernels.tuning(SLM_LINEAR_RT=4, SLM_LINEAR_NW=4, SLM_LINEAR_SPLITK=1):   # the dense knobs do not reach it
        assert bytes(ref.host_plan(ref.host_args(8, 4096, 4096))[1]) == bytes(base)
    with kernels.tuning(SLM_W4A4_RT=4, SLM_W4A4_NW=1, SLM_W4A4_SPLITK=5):
        info = ref.host_plan(ref.host_args(8, 256, 64))[1]
        assert (info.row_tiles, info.waves, info.split_k) == (4, 4, 2)             # waves >= row tiles; chunks cap
        assert ref.host_plan(ref.host_args(8, 4096, 128, flags=SILU))[1].split_k == 1


def test_validation_precedes_any_launch():
    """host address 4096 stands for every pointer: no call may reach a kernel"""
    L = _lib.lib()
    F = lambda g: L.slm_w4a4_linear(C.byref(g), None)  # noqa: E731
    A = ref.host_args
    assert L.slm_w4a4_linear(None, None) == INVALID
    for g in (A(8, 4096 + 16, 4096), A(8, 4096, 4096 + 16), A(8, 4096, 4096 + 32, flags=SILU),   # K % 32, N % 32, N % 64
              A(8, 4096, 4096, dtype=_lib.SLM_F32)):
        assert F(g) == UNSUPPORTED
    for g in (A(8, 4096, 4096, flags=SILU | DEFER), A(8, 4096, 4096, flags=64), A(-1, 4096, 4096)):
        assert F(g) == INVALID
    for q in (False, True):
        full = 2048 if q else 4096                                      # lda: bytes of codes / elements of T
        muts = [(dict(lda=full - 8), INVALID), (dict(lda=full + 8), ALIGNMENT if q else WORKSPACE),   # codes: lda % 16
                (dict(lda=full + 1), ALIGNMENT), (dict(a=4096 + 8), ALIGNMENT), (dict(ldw=2032), INVALID),
                (dict(ldw=2048 + 8), ALIGNMENT), (dict(w_scale=None), INVALID), (dict(lds=127), INVALID),
                (dict(lds=129, w_scale=4096 + 3), WORKSPACE),            # scales: no alignment; a valid split plan
                (dict(ldc=4088), INVALID), (dict(ldc=4096 + 1), ALIGNMENT), (dict(a=None), INVALID),
                (dict(w=None), INVALID), (dict(c=None), INVALID)]
        if q:
            muts += [(dict(ldas=127), INVALID), (dict(ldas=131, a_scale=4096 + 5), WORKSPACE)]
        for mut, code in muts:
            assert F(A(8, 4096, 4096, quantised=q, **mut)) == code, (q, mut)
        assert F(A(0, 4096, 4096, quantised=q, a=None, c=None)) == 0    # M == 0: a no-op
    g = A(8, 4096, 4096)
    info = ref.host_plan(g)[1]
    g.workspace, g.workspace_bytes = 4096, info.workspace_bytes - 1
    assert info.split_k > 1 and F(g) == WORKSPACE
    assert L.slm_w4a4_linear_plan(C.byref(g), None) == INVALID
    Q = L.slm_w4a4_quantize_act      # (a, lda, aq, ldaq, a_scale, ldas, M, K, dtype, stream)
    ok = dict(a=4096, lda=64, aq=8192, ldaq=32, s=12288, ldas=2, M=4, K=64, dt=1)
    for mut, code in ((dict(K=48), UNSUPPORTED), (dict(dt=2), UNSUPPORTED), (dict(lda=56), INVALID), (dict(s=None), INVALID),
                      (dict(ldas=1), INVALID), (dict(ldaq=40), ALIGNMENT), (dict(lda=68), ALIGNMENT),
                      (dict(M=0, a=None, aq=None, s=None), 0)):
        assert Q(*dict(ok, **mut).values(), None) == code, mut
