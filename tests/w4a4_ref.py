"""What the MXFP4 x MXFP4 linear tests share (include/slm_hip.h section 22, slm_w4a4_linear): the float64 reference
over two MXFP4 operands, exactly representable inputs, the case table, the knobs and the ctypes block of a CPU query.
The value table, pack / unpack, rounding and the GEMM tolerance are tests/mxfp4_ref.py's and tests/dense_ref.py's."""
import ctypes as C

import numpy as np
import torch

from .mxfp4_ref import (BLOCK, DTYPES, E2M1, EXACT_SCALES, FORMS, GEMM_TOL, INT_CODES, as64, code_sweep,  # noqa: F401
                        linear_ref, pack, rel_err, rounded, torch_dtype, unpack, w_as64)

AX_K = (32, 96, 128, 160, 672, 1312)   # tail only (x2), one chunk, chunk + one unit, ring wrap + one unit, wrap + 3 units
AX_N = (32, 96, 160)
AX_M = (1, 31, 33, 65, 129)
_SPLITS = ((1, 1, 1, 1, 3, 2), (1, 1, 1, 1, 5, 3))   # by K: what its chunk count allows


def exact_cases():
    """(M, N, K, rt, nw, split, with_bias): every K per form; M, N, the split and the bias rotate from form to form"""
    cases = []
    for fi, (rt, nw) in enumerate(FORMS):
        for i, K in enumerate(AX_K):
            cases.append((AX_M[(i + fi) % len(AX_M)], AX_N[(i + 2 * fi) % len(AX_N)], K, rt, nw, _SPLITS[fi % 2][i],
                          (i + fi) % 2 == 0))
    return cases


EXACT_CASES = exact_cases()
CORNERS = ((1, 32, 32, 1), (33, 96, 672, 1), (129, 160, 1312, 2))   # (M, N, K, split)


def knobs(rt, nw, split):
    return dict(SLM_W4A4_RT=rt, SLM_W4A4_NW=nw, SLM_W4A4_SPLITK=split)


def w4a4_ref(aq, a_scale, wq, w_scale, bias64=None, k_range=None):
    """dequant(A) . dequant(W)^T (+ bias) in float64, optionally over k in [k0, k1) only"""
    return linear_ref(w_as64(aq, a_scale), w_as64(wq, w_scale), bias64, k_range)


def int_inputs(rng, M, K, N, with_bias):
    """both operands codes of {0, +-1, +-2, +-3, +-4, +-6} under block scales 2^-2 .. 2^1, bias in [-8, 8]: every
    product is a multiple of 1/16 below 144 in magnitude, so with K <= 1312 every partial sum is a multiple of 1/16
    below 2^18 (144 * 1312 + 8 = 188936): exact in fp32 in ANY order, the result one rounding of float64.  Returns
    aq [M, K/2], a_scale [M, K/32], wq [N, K/2], w_scale [N, K/32] (uint8 CPU tensors), bias64."""
    def operand(rows):
        return (pack(rng.choice(INT_CODES, size=(rows, K))),
                torch.from_numpy(rng.choice(EXACT_SCALES, size=(rows, K // BLOCK)).astype(np.uint8)))
    aq, asc = operand(M)
    wq, wsc = operand(N)
    b = rng.integers(-8, 9, size=(N,)).astype(np.float64) if with_bias else None
    return aq, asc, wq, wsc, b


def one_hot(rows, K, offset, e_lo=121, span=7):
    """(codes [rows, K/2], scale [rows, K/32]): row r holds 1.0 (code 2) at k = r % 32 + offset and zeros elsewhere;
    the scale byte of block (r, b) is e_lo + (r + 3 b) mod span: distinct along a row and down a column"""
    codes = np.zeros((rows, K), dtype=np.int64)
    codes[np.arange(rows), np.arange(rows) % 32 + offset] = 2
    scale = e_lo + (np.arange(rows)[:, None] + 3 * np.arange(K // BLOCK)[None, :]) % span
    return pack(codes), torch.from_numpy(scale.astype(np.uint8))


def host_args(M, K, N, bits="bf16", flags=0, bias=False, quantised=False, **kw):
    """slm_w4a4_linear_args for a host-side query: address 4096 stands for every pointer"""
    from scalellm_amd import _lib
    g = _lib.W4A4LinearArgs()
    g.a = g.w = g.c = g.w_scale = 4096
    g.bias = 4096 if bias else None
    g.a_scale = 4096 if quantised else None
    g.M, g.K, g.N = M, K, N
    g.lda, g.ldw, g.lds, g.ldas = (K // 2 if quantised else K), K // 2, K // 32, K // 32
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
    return _lib.lib().slm_w4a4_linear_plan(C.byref(g), C.byref(info)), info
