"""What the fp8 grouped GEMM tests share (include/slm_hip.h section 16, slm_moe_fp8_gemm): the float64 reference on
the e4m3 values themselves (e4m3 -> float64 is exact, so no quantisation error enters a comparison), the routing /
aligned-list helpers of tests/moe_dense_ref.py, and the case tables.  Tolerances are the project's own: GEMM_TOL for
one GEMM on random inputs, twice that for SiLU products and for the layer's two chained GEMMs."""
import numpy as np

from . import fp8_ref
from . import moe_dense_ref as dref
from . import moe_ref
from .fp8_ref import SCALE_CHOICES, code_sweep_weight, e4m3_value, to_w8, w8_as64  # noqa: F401
from .moe_dense_ref import (GEMM_TOL, PROJECT_CASES, PROJECT_E, PROJECT_TOPK, aligned, as64, rel_err,  # noqa: F401
                            rounded, routing, torch_dtype)


def grouped_fp8_ref(a64, w8, scale64, ids, a_div):
    """per flat index f = t * k + j, e = ids[f]:  (A[f // a_div] @ e4m3(W8[e]).T) * scale[e]  in float64 ->
    [n_flat, N].  w8: [E, N, K] float8_e4m3fn / uint8 tensor, or its float64 values; scale64: [E, N] or None"""
    w64 = w8 if isinstance(w8, np.ndarray) else w8_as64(w8)
    out = dref.grouped_ref(a64, w64, ids, a_div)
    if scale64 is not None:
        out = out * np.asarray(scale64, dtype=np.float64)[np.asarray(ids).reshape(-1)]
    return out


# ---- the case tables -------------------------------------------------------------------------------------------------
# (K, N, E, T, k) of the same-bits test: 5 chunks (the ring wraps, an odd count) with a part-filled last column group,
# and 3 chunks + 3 tail units; T = 33 under crowded routing spills into a second block
SAME_BITS_CASES = ((640, 160, 8, 33, 2), (480, 96, 4, 33, 2))
SAME_BITS_SILU = (640, 320, 8, 33, 2)
# expert_ids.numel() sizes the grid and, with N, decides the waves per workgroup (moe_gemm_waves): at N = 160
# (SiLU * mul: N = 320) None = the capacity rule -> NW = 1 (SiLU: 2), 100 blocks -> 2 (SiLU: 4), 128 blocks -> 4
LAUNCH_BLOCKS = (None, 100, 128)
EXACT_CASE = (640, 160, 8, 33, 2)
TAIL_KS = (32, 96, 160, 480)                 # tail units only; chunks, then one and three tail units
TAIL_CASE = (96, 4, 33, 2)                   # N, E, T, k
SILU_CASES = ((128, 64, 1, 3, 1), (384, 128, 8, 33, 2), (640, 320, 8, 96, 4))   # K, N, E, T, k
MOE_LAYER = dict(hidden=256, intermediate=384, n_experts=8, topk=2)
MOE_TOKENS = (1, 5, 70)

MI355X_CUS = 256


def launch_waves(max_blocks, N, silu):
    """moe_gemm_waves of csrc/moe_gemm_plan.h restated: the widest of 4, 2, 1 waves (SiLU * mul: 4, 2) that still
    yields one workgroup per CU, otherwise the narrowest"""
    n_tiles = N // 32
    narrowest = 2 if silu else 1
    nw = 4
    while nw > narrowest:
        groups = (n_tiles // 2 + nw // 2 - 1) // (nw // 2) if silu else (n_tiles + nw - 1) // nw
        if max_blocks * groups >= MI355X_CUS:
            return nw
        nw //= 2
    return narrowest


def blocks_of(blocks, n_flat, E):
    return moe_ref.align_capacity(n_flat, E, 32)[1] if blocks is None else blocks


def quantized_experts(rng, E, N, K):
    """randn experts quantised per output channel by kernels.quantize_fp8_weight: (w8 [E, N, K], scale fp32 [E, N])"""
    import torch
    from scalellm_amd import kernels
    w = torch.from_numpy(rng.standard_normal((E * N, K)).astype(np.float32))
    w8, scale = kernels.quantize_fp8_weight(w, "channel")
    return w8.view(torch.uint8).view(E, N, K).view(torch.float8_e4m3fn), scale.view(E, N).contiguous()


def int_experts(rng, E, N, K):
    """integer weights |w| <= 3: e4m3 numbers (asserted by to_w8), [E, N, K] float8_e4m3fn"""
    return fp8_ref.to_w8(rng.integers(-3, 4, size=(E, N, K)).astype(np.float64))
