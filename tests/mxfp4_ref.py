"""What the MXFP4 linear tests share (include/slm_hip.h section 20, slm_mxfp4_linear): the e2m1 value table written
out from the format, the unpack (a byte's low nibble is the lower k), the float64 reference, the case tables and the
ctypes argument block of a CPU query.  Forms, exact cases, knobs, rounding and the GEMM tolerance are
tests/dense_ref.py's; the same-bits and random cases are tests/fp8_ref.py's (every K there is a multiple of 32; 672
and 1312 give the odd scale-row lengths 21 and 41 and tail units)."""
import ctypes as C

import numpy as np
import torch

from .dense_ref import (DTYPES, EXACT_CASES, FORMS, GEMM_TOL, SPLITS, as64, knobs, linear_ref,  # noqa: F401
                        rel_err, rounded, silu_mul_ref, torch_dtype)
from .fp8_ref import RANDOM_CASES, SAME_BITS_CASES, SAME_BITS_SILU  # noqa: F401

BLOCK = 32
# OCP e2m1: 1 sign, 2 exponent (bias 1), 1 mantissa bit; code = S.EE.M.  E = 0 is subnormal (M / 2), else
# (1 + M / 2) 2^(E - 1): no infinity, no NaN
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])
# the codes of the integers the exact tests draw from: {0, +-1, +-2, +-3, +-4, +-6}
INT_CODES = np.array([0, 2, 4, 5, 6, 7, 10, 12, 13, 14, 15])
EXACT_SCALES = (125, 126, 127, 128)


def unpack(packed):
    """uint8 [N, K/2] (numpy or torch) -> codes int64 numpy [N, K]: byte b holds k = 2 b (low nibble) and 2 b + 1"""
    p = packed.detach().cpu().numpy() if isinstance(packed, torch.Tensor) else np.asarray(packed)
    p = p.astype(np.int64)
    out = np.empty((p.shape[0], 2 * p.shape[1]), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = p & 0xF, p >> 4
    return out


def pack(codes):
    """codes [N, K] in 0..15 -> uint8 CPU tensor [N, K/2], the low nibble first"""
    c = np.asarray(codes, dtype=np.int64)
    return torch.from_numpy((c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8))


def w_as64(packed, scale):
    """e2m1(code) * 2^(e - 127) in float64 [N, K]: exact (a 2-bit significand times a power of two)"""
    s = scale.detach().cpu().numpy() if isinstance(scale, torch.Tensor) else np.asarray(scale)
    e = np.repeat(s.astype(np.int64), BLOCK, axis=1)
    return E2M1[unpack(packed)] * np.exp2((e - 127).astype(np.float64))


def mxfp4_ref(a64, packed, scale, bias64=None, k_range=None):
    """A . dequant(W)^T (+ bias) in float64, optionally over k in [k0, k1) only"""
    return linear_ref(a64, w_as64(packed, scale), bias64, k_range)


def int_inputs(rng, M, K, N, with_bias):
    """a integers in [-4, 4], W codes of {0, +-1, +-2, +-3, +-4, +-6} under block scales 2^-2 .. 2^1, bias in
    [-8, 8]: every product is a multiple of 1/4 below 48 in magnitude, so with K <= 1312 every partial sum is a
    multiple of 1/4 below 2^16 (48 * 1312 + 8 = 62984): exact in fp32 in ANY order, and the result is one rounding of
    the float64 reference.  Returns a64, packed uint8 [N, K/2], scale uint8 [N, K/32], bias64."""
    a = rng.integers(-4, 5, size=(M, K)).astype(np.float64)
    codes = rng.choice(INT_CODES, size=(N, K))
    scale = rng.choice(EXACT_SCALES, size=(N, K // BLOCK)).astype(np.uint8)
    b = rng.integers(-8, 9, size=(N,)).astype(np.float64) if with_bias else None
    return a, pack(codes), torch.from_numpy(scale), b


def code_sweep(n=256, k=256):
    """(packed [n, k/2], scale [n, k/32]): the nibble of W[n, k] is (n + k) mod 16, the scale byte of block
    (n, k / 32) is 114 + (n + k / 32) mod 27 -- exact in both dtypes, and all eight blocks of a row differ"""
    codes = (np.arange(n)[:, None] + np.arange(k)[None, :]) % 16
    scale = 114 + (np.arange(n)[:, None] + np.arange(k // BLOCK)[None, :]) % 27
    return pack(codes), torch.from_numpy(scale.astype(np.uint8))


def host_args(M, K, N, bits="bf16", flags=0, bias=False, **kw):
    """slm_mxfp4_linear_args for a host-side query: address 4096 stands for every pointer (never dereferenced)"""
    from scalellm_amd import _lib
    g = _lib.Mxfp4LinearArgs()
    g.a = g.w = g.c = g.w_scale = 4096
    g.bias = 4096 if bias else None
    g.M, g.K, g.N = M, K, N
    g.lda, g.ldw, g.lds = K, K // 2, K // 32
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
    rc = _lib.lib().slm_mxfp4_linear_plan(C.byref(g), C.byref(info))
    return rc, info
