"""CPU tests of the MXFP4-producing entries (include/slm_hip.h section 24): declared, exported and bound; validation
before any launch (host address 4096 stands for every pointer: no call may reach a kernel)."""
import ctypes as C
import re
import subprocess

import pytest

from scalellm_amd import _lib, kernels

from . import w4a4_ref as ref
from .test_w4a4_cpu import ALIGNMENT, DEFER, HEADER, INVALID, SILU, UNSUPPORTED

SYMBOLS = ["slm_rms_norm_mxfp4", "slm_rms_norm_mxfp4_splitk", "slm_w4a4q_linear", "slm_w4a4q_linear_plan"]


def test_the_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"SLM_API\s+[\w\s\*]+?\b(slm_\w+)\s*\(", src))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for n in SYMBOLS:
        assert n in declared and re.search(rf"\sT\s+{n}\n", exported), n
        assert getattr(_lib.lib(), n).argtypes is not None, n
    assert callable(kernels.rms_norm_mxfp4)


# (aq, ldaq, a_scale, ldas, out_t, x | partials [, n_splits], weight, residual, n_tokens, dim, eps, dtype)
NORM_OK = dict(aq=4096, ldaq=2048, s=4096, ldas=128, out=None, x=4096, w=4096, res=None, T=4, dim=4096, eps=1e-5, dt=1)
NORM_CASES = [(dict(dim=4096 + 8), UNSUPPORTED), (dict(dim=16384 + 32, ldaq=1 << 14, ldas=1 << 10), UNSUPPORTED),
              (dict(dt=2), UNSUPPORTED), (dict(ldaq=2032), INVALID), (dict(ldaq=2056), ALIGNMENT), (dict(ldas=127), INVALID),
              (dict(aq=None), INVALID), (dict(s=None), INVALID), (dict(x=None), INVALID), (dict(w=None), INVALID),
              (dict(aq=4096 + 8), ALIGNMENT), (dict(out=4096 + 2), ALIGNMENT), (dict(splits=0), INVALID), (dict(splits=0, T=0), 0),
              (dict(T=0, aq=None, s=None, x=None, w=None), 0)]


@pytest.mark.parametrize("mut,code", NORM_CASES, ids=[",".join(m) for m, _ in NORM_CASES])
def test_the_norm_validates_before_any_launch(mut, code):
    L, a = _lib.lib(), {**NORM_OK, "splits": 3, **mut}
    head, tail = (a["aq"], a["ldaq"], a["s"], a["ldas"], a["out"]), (a["w"], a["res"], a["T"], a["dim"], a["eps"], a["dt"], None)
    assert L.slm_rms_norm_mxfp4_splitk(*head, a["x"], a["splits"], *tail) == code
    if "splits" not in mut:
        assert L.slm_rms_norm_mxfp4(*head, a["x"], *tail) == code


def _q(M=8, K=4096, N=4096, flags=SILU, **kw):
    return ref.host_args(M, K, N, flags=flags, **dict(dict(ldc=N // 4), **kw))


QOUT_CASES = [(_q(flags=0), 4096, 64, INVALID), (_q(flags=SILU | DEFER), 4096, 64, INVALID), (_q(bias=True), 4096, 64, INVALID),
              (_q(), None, 64, INVALID), (_q(ldc=1024 + 8), 4096, 64, ALIGNMENT), (_q(ldc=1008), 4096, 64, INVALID),
              (_q(), 4096, 63, INVALID), (_q(N=4096 + 32), 4096, 65, UNSUPPORTED), (_q(quantised=True, ldas=127), 4096, 64, INVALID),
              (_q(M=0, a=None, c=None), None, 0, 0)]


@pytest.mark.parametrize("g,c_scale,ldcs,code", QOUT_CASES, ids=[str(i) for i in range(len(QOUT_CASES))])
def test_the_quantising_gemm_validates_before_any_launch(g, c_scale, ldcs, code):
    L = _lib.lib()
    assert L.slm_w4a4q_linear(C.byref(g), c_scale, ldcs, None) == code
    assert L.slm_w4a4q_linear(None, 4096, 64, None) == INVALID


def test_the_quantising_gemm_plans_as_the_plain_one():
    g, info = _q(M=40), _lib.LinearPlanInfo()
    assert _lib.lib().slm_w4a4q_linear_plan(C.byref(g), C.byref(info)) == 0
    assert bytes(info) == bytes(ref.host_plan(g)[1]) and info.split_k == 1 and info.waves >= 2
    assert _lib.lib().slm_w4a4q_linear_plan(C.byref(_q(flags=0)), C.byref(info)) == INVALID
