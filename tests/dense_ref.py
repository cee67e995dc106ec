"""What the dense linear tests share (include/slm_hip.h section 13, slm_linear): the float64 numpy reference,
exactly representable inputs, the case table of the exact test and the ctypes argument block of a CPU query."""
import ctypes as C

import numpy as np

from .moe_dense_ref import GEMM_TOL, as64, rel_err, rounded, torch_dtype  # noqa: F401 (re-exported)

DTYPES = ("f16", "bf16")


def linear_ref(a64, w64, bias64=None, k_range=None):
    """A[M, K] . W[N, K]^T (+ bias) in float64, optionally over k in [k0, k1) only"""
    if k_range is not None:
        a64, w64 = a64[:, k_range[0]:k_range[1]], w64[:, k_range[0]:k_range[1]]
    out = a64 @ w64.T
    return out if bias64 is None else out + bias64[None, :]


def silu_mul_ref(y64):
    """silu(gate) * up over [M, gate | up] in float64"""
    d = y64.shape[1] // 2
    g, u = y64[:, :d], y64[:, d:]
    return g / (1.0 + np.exp(-g)) * u


def int_inputs(rng, M, K, N, with_bias):
    """a, W integers in [-4, 4], bias in [-8, 8]: with K <= 1312 every partial sum is below 2^24 in magnitude
    (16 * 1312 + 8 = 21000), so fp32 accumulation is exact in ANY order and the result is one rounding of the
    float64 reference"""
    a = rng.integers(-4, 5, size=(M, K)).astype(np.float64)
    w = rng.integers(-4, 5, size=(N, K)).astype(np.float64)
    b = rng.integers(-8, 9, size=(N,)).astype(np.float64) if with_bias else None
    return a, w, b


# ---- the exact test's table -------------------------------------------------------------------------------------
# kernel forms: (row tiles per wave, waves per workgroup); the kernel needs waves >= row tiles (csrc/dense.hip)
FORMS = ((1, 1), (1, 2), (1, 4), (2, 2), (2, 4), (4, 4))
SPLITS = (1, 2, 3, 5)
AX_M = (1, 2, 31, 32, 33, 64, 65, 96, 128, 129, 160)
AX_N = (32, 96, 160)
AX_K = (32, 96, 128, 256, 640, 672, 1312)   # tail only (x2), a ring shorter than its depth (x2), wrap, wrap + 1 / + 3 tail units
# eleven rows per form: every K, and with it a split that K's chunk count allows (K / 128 >= split)
_K_SEQ = (32, 96, 128, 256, 640, 672, 1312, 640, 1312, 672, 256)
_S_SEQ = (1, 1, 1, 2, 5, 3, 2, 1, 3, 5, 1)


def exact_cases():
    """(M, N, K, rt, nw, split, with_bias): per form every value of every axis, every split; the M / N / K pairings
    rotate from form to form"""
    cases = []
    for fi, (rt, nw) in enumerate(FORMS):
        for i in range(len(AX_M)):
            cases.append((AX_M[(i + 3 * fi) % len(AX_M)], AX_N[(i + fi) % len(AX_N)], _K_SEQ[i], rt, nw, _S_SEQ[i],
                          (i + fi) % 2 == 0))
    return cases


EXACT_CASES = exact_cases()


def knobs(rt, nw, split):
    return dict(SLM_LINEAR_RT=rt, SLM_LINEAR_NW=nw, SLM_LINEAR_SPLITK=split)


def host_args(M, K, N, bits="bf16", flags=0, bias=False, **kw):
    """slm_linear_args for a host-side query: address 4096 stands for every pointer (never dereferenced)"""
    from scalellm_amd import _lib
    g = _lib.LinearArgs()
    g.a = g.w = g.c = 4096
    g.bias = 4096 if bias else None
    g.M, g.K, g.N = M, K, N
    g.lda, g.ldw = K, K
    g.ldc = N // 2 if flags & _lib.SLM_LINEAR_SILU_MUL else N
    g.dtype = _lib.SLM_BF16 if bits == "bf16" else _lib.SLM_F16
    g.flags = flags
    g.workspace, g.workspace_bytes = None, 0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def host_plan(g):
    from scalellm_amd import _lib
    info = _lib.LinearPlanInfo()
    rc = _lib.lib().slm_linear_plan(C.byref(g), C.byref(info))
    return rc, info
