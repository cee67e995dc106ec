"""What the fp8 x fp8 linear tests share (include/slm_hip.h section 25); e4m3 helpers and tolerance: fp8_ref, moe_dense_ref."""
import ctypes as C

import numpy as np
import torch

from . import fp8_ref
from .fp8_ref import DTYPES, as64, code_sweep_weight, linear_ref, rel_err, rounded, to_w8, torch_dtype, w8_as64  # noqa: F401
from .moe_dense_ref import GEMM_TOL  # noqa: F401

FORMS = ((1, 1), (2, 2), (4, 4))
INT_CASES = ((33, 96, 672, 1), (5, 32, 1312, 3), (130, 160, 160, 1))


def knobs(rt, nw, split):
    return dict(SLM_W8A8_RT=rt, SLM_W8A8_NW=nw, SLM_W8A8_SPLITK=split)


def quant_ref(a, static_scale=None):
    """section 25's rule on the CPU: (codes uint8 [M, K], scale fp32 [M])"""
    x = a.detach().cpu().float()
    amax = x.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    s = torch.where(torch.isfinite(amax), s, torch.full_like(s, float("nan")))
    if static_scale is not None:
        s = torch.full_like(s, float(static_scale))
    return (x / s[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8), s


def w8a8_ref(aq, a_scale, w8, w_scale, bias64=None, k_range=None):
    """((e4m3(Aq) . e4m3(W8)^T) * a_scale[:, None]) * w_scale[None, :] (+ bias) in float64"""
    y = linear_ref(w8_as64(aq), w8_as64(w8), None, k_range) * as64(a_scale)[:, None] * as64(w_scale)[None, :]
    return y if bias64 is None else y + bias64[None, :]


def int_inputs(rng, M, K, N):
    """integers in [-16, 16] (exact in e4m3), power-of-two scales (outputs of a few units), an integer bias: every partial
    sum is an integer < 2^24 times a power of two, exact in fp32 in ANY order.  aq, a_scale, w8, w_scale (CPU), bias64."""
    aq, w8 = to_w8(rng.integers(-16, 17, size=(M, K))), to_w8(rng.integers(-16, 17, size=(N, K)))
    a_scale = torch.from_numpy(2.0 ** rng.integers(-9, -6, size=(M,))).float()
    w_scale = torch.from_numpy(2.0 ** rng.integers(-2, 2, size=(N,))).float()
    return aq, a_scale, w8, w_scale, rng.integers(-8, 9, size=(N,)).astype(np.float64)


def one_hot(rows, K, offset):
    """e4m3 [rows, K]: row r holds 1.5 at k = (r % 32 + offset) % K and zeros elsewhere"""
    x = np.zeros((rows, K))
    x[np.arange(rows), (np.arange(rows) % 32 + offset) % K] = 1.5
    return to_w8(x)


def host_args(M, K, N, bits="bf16", flags=0, **kw):
    """slm_w8a8_linear_args for a host-side query: fp8_ref.host_args' block (address 4096 for every pointer) + a_scale"""
    from scalellm_amd import _lib
    f, g = fp8_ref.host_args(M, K, N, bits, flags), _lib.W8A8LinearArgs()
    for name, _ in _lib.Fp8LinearArgs._fields_:
        setattr(g, name, getattr(f, name))
    g.a_scale = 4096
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def host_plan(g):
    from scalellm_amd import _lib
    info = _lib.LinearPlanInfo()
    return _lib.lib().slm_w8a8_linear_plan(C.byref(g), C.byref(info)), info
