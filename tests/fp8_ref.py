"""What the fp8 linear tests share (include/slm_hip.h section 15, slm_fp8_linear): the float64 reference (e4m3 ->
float64 is exact), the e4m3 code table, the case tables and the ctypes argument block of a CPU query.  Forms, exact
cases, knobs, rounding and the GEMM tolerance are tests/dense_ref.py's."""
import ctypes as C

import numpy as np
import torch

from .dense_ref import (DTYPES, EXACT_CASES, FORMS, GEMM_TOL, SPLITS, as64, int_inputs, knobs, linear_ref,  # noqa: F401
                        rel_err, rounded, silu_mul_ref, torch_dtype)

# (M, N, K, rt, nw, split): the forced forms of the same-bits test and of the slab test
SAME_BITS_CASES = ((33, 96, 1312, 2, 2, 3), (1, 160, 672, 1, 4, 5), (129, 32, 640, 4, 4, 2))
SAME_BITS_SILU = (40, 192, 672, 2, 2, 1)
RANDOM_CASES = ((1, 4096, 512), (32, 1024, 256), (160, 512, 96))   # (M, K, N)
SCALE_CHOICES = (0.25, 0.5, 1.0, 2.0)


def e4m3_value(code):
    """float64 value of OCP e4m3fn code(s): 1 sign, 4 exponent (bias 7), 3 mantissa bits, no infinities; S.1111.111
    is NaN.  Written out from the format, independent of torch's conversion."""
    code = np.asarray(code, dtype=np.int64)
    sign = np.where(code & 0x80, -1.0, 1.0)
    e, m = (code >> 3) & 0xF, code & 0x7
    val = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1.0 + m / 8.0) * 2.0 ** (e.astype(np.float64) - 7.0))
    return np.where((code & 0x7F) == 0x7F, np.nan, sign * val)


def w8_as64(w8):
    """float8_e4m3fn (or its bytes) -> float64 numpy, exact"""
    t = w8 if w8.dtype == torch.float8_e4m3fn else w8.view(torch.float8_e4m3fn)
    return t.detach().cpu().to(torch.float32).double().numpy()


def to_w8(w64):
    """float64 values that ARE e4m3 numbers -> float8_e4m3fn CPU tensor (asserted exact)"""
    t = torch.from_numpy(np.ascontiguousarray(w64, dtype=np.float64)).to(torch.float32).to(torch.float8_e4m3fn)
    assert np.array_equal(w8_as64(t), np.asarray(w64, dtype=np.float64)), "not representable in e4m3"
    return t


def fp8_ref(a64, w8, scale64=None, bias64=None, k_range=None):
    """(A . e4m3(W8)^T) * scale (+ bias) in float64, optionally over k in [k0, k1) only"""
    w64 = w8 if isinstance(w8, np.ndarray) else w8_as64(w8)
    y = linear_ref(a64, w64, None, k_range)
    if scale64 is not None:
        y = y * np.asarray(scale64, dtype=np.float64)[None, :]
    return y if bias64 is None else y + bias64[None, :]


def code_sweep_weight(n=256, k=256):
    """W[n, k] = code (n + k) mod 256 with the two NaN codes replaced by 0: uint8 [n, k]"""
    codes = (np.arange(n)[:, None] + np.arange(k)[None, :]) % 256
    codes = np.where((codes & 0x7F) == 0x7F, 0, codes)
    return torch.from_numpy(codes.astype(np.uint8))


def host_args(M, K, N, bits="bf16", flags=0, bias=False, scale=True, **kw):
    """slm_fp8_linear_args for a host-side query: address 4096 stands for every pointer (never dereferenced)"""
    from scalellm_amd import _lib
    g = _lib.Fp8LinearArgs()
    g.a = g.w = g.c = 4096
    g.bias = 4096 if bias else None
    g.w_scale = 4096 if scale else None
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
    rc = _lib.lib().slm_fp8_linear_plan(C.byref(g), C.byref(info))
    return rc, info
