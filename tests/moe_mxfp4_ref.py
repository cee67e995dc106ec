"""What the MXFP4 grouped GEMM tests share (include/slm_hip.h section 21, slm_moe_mxfp4_gemm): the float64 reference
on the e2m1 * 2^(e - 127) values themselves (exact, so no quantisation error enters a comparison), expert-stacked
forms of tests/mxfp4_ref.py's generators, the routing / aligned-list helpers of tests/moe_dense_ref.py and the launch
shapes of tests/moe_fp8_ref.py, and the case tables.  Nothing here has a tolerance: every GPU comparison is bit for
bit, against the dense grouped GEMM on the dequantised experts or against one rounding of the float64 value."""
import ctypes as C

import numpy as np
import torch

from . import moe_dense_ref as dref
from . import mxfp4_ref as mref
from .moe_dense_ref import aligned, as64, rounded, routing, torch_dtype  # noqa: F401
from .moe_fp8_ref import blocks_of, launch_waves  # noqa: F401
from .mxfp4_ref import BLOCK, E2M1  # noqa: F401


def experts_as64(packed, scale):
    """uint8 [E, N, K/2] and [E, N, K/32] -> float64 [E, N, K], exact"""
    return np.stack([mref.w_as64(packed[e], scale[e]) for e in range(packed.shape[0])])


def grouped_mxfp4_ref(a64, packed, scale, ids, a_div):
    """per flat index f = t * k + j, e = ids[f]:  A[f // a_div] @ dequant(W[e]).T  in float64 -> [n_flat, N]"""
    return dref.grouped_ref(a64, experts_as64(packed, scale), ids, a_div)


def random_experts(rng, E, N, K, scale_lo=118, scale_hi=126):
    """every code, scale bytes in [scale_lo, scale_hi]: 118..126 is exact in bf16 AND f16.
    (packed uint8 [E, N, K/2], scale uint8 [E, N, K/32])"""
    packed = torch.from_numpy(rng.integers(0, 256, size=(E, N, K // 2), dtype=np.uint8))
    scale = torch.from_numpy(rng.integers(scale_lo, scale_hi + 1, size=(E, N, K // BLOCK)).astype(np.uint8))
    return packed, scale


def dequantized(packed, scale, bits):
    """the [E, N, K] tensor of T the dense kernel takes: kernels.dequantize_mxfp4_weight per expert, checked exact"""
    from scalellm_amd import kernels
    E, N = packed.shape[:2]
    w = kernels.dequantize_mxfp4_weight(packed.reshape(E * N, -1), scale.reshape(E * N, -1), torch_dtype(bits))
    assert np.array_equal(as64(w), experts_as64(packed, scale).reshape(E * N, -1))   # exact in T
    return w.view(E, N, -1)


def int_experts(rng, E, M, K, N):
    """mxfp4_ref.int_inputs per expert (its docstring has the exactness argument; K <= 1312): a64 [M, K] of the first
    draw, packed [E, N, K/2], scale [E, N, K/32]"""
    a, ps, ss = None, [], []
    for _ in range(E):
        a_e, p, s, _ = mref.int_inputs(rng, M, K, N, False)
        a = a_e if a is None else a
        ps.append(p)
        ss.append(s)
    return a, torch.stack(ps), torch.stack(ss)


def code_sweep_experts(E, N, K):
    """mxfp4_ref.code_sweep with the code offset by the expert id: the nibble of W[e][n, k] is (e + n + k) mod 16, the
    scale byte of block (e, n, b) 114 + (e + n + b) mod 27"""
    p, s = mref.code_sweep(N + E, K)
    return torch.stack([p[e:e + N] for e in range(E)]), torch.stack([s[e:e + N] for e in range(E)])


def scale_pattern(E, N, nb, bits):
    """the scale byte of block (e, n, b): 100 + (37 e + 5 n + b) mod 101 (bf16: 2^-27 .. 2^73) or 114 + (...) mod 27
    (f16: 2^-13 .. 2^13).  With nb <= 5 no two of (e, n, b), (e, n + 1, b'), (e + 1, n, b') share a byte: the steps are
    1, 5 and 37 (10 mod 27), and 5 - (b - b'), 37 - (b - b'), 10 - (b - b') are never 0 for |b - b'| <= 4."""
    assert nb <= 5
    v = 37 * np.arange(E)[:, None, None] + 5 * np.arange(N)[None, :, None] + np.arange(nb)[None, None, :]
    s = 100 + v % 101 if bits == "bf16" else 114 + v % 27
    return torch.from_numpy(s.astype(np.uint8))


# ---- the case tables -------------------------------------------------------------------------------------------------
# K: tail units only (no chunk); one chunk (every ring load clamped); chunk + one tail unit; three chunks + a tail
# unit (one full ring turn); five chunks + a tail unit with a scale row of 21 bytes
SAME_BITS_KS = (96, 128, 160, 416, 672)
SAME_BITS_NS = (32, 64, 160)
SAME_BITS_E, SAME_BITS_T, SAME_BITS_TOPK = 8, 33, 2
# expert_ids.numel() sizes the grid and, with N, decides the waves per workgroup (moe_gemm_waves).  N = 160: None = the
# capacity rule -> NW = 1, 100 blocks -> 2, 128 blocks -> 4 (tests/moe_fp8_ref.py).  N = 32 / 64 are one column group
# at every width: the capacity rule -> 1, 256 blocks -> 4 (three or two of the four waves on clamped duplicate tiles).
LAUNCH_BLOCKS = {32: (None, 256), 64: (None, 256), 160: (None, 100, 128)}
# SiLU * mul needs (N / 2) % 32 == 0: of the three only N = 64 (NW = 2, and 4 from 256 blocks); N = 192 adds a
# part-filled pair group (three output tiles: NW = 2, 2 at 100 blocks, 4 at 128)
SILU_BLOCKS = {64: (None, 256), 192: (None, 100, 128)}
MOE_LAYER = dict(hidden=256, intermediate=384, n_experts=8, topk=2)
MOE_TOKENS = (1, 5, 70)


def host_args(K0=256, N0=128, **kw):
    """slm_moe_mxfp4_gemm_args for a host-side call over a dense [K0, N0] problem, fields overridden by name: address
    4096 stands for every pointer (never dereferenced)"""
    from scalellm_amd import _lib
    K, N = K0, N0
    g = _lib.MoeMxfp4GemmArgs()
    g.a = g.w = g.w_scale = g.c = g.sorted_token_idxes = g.expert_ids = g.n_padded_tokens = 4096
    g.K, g.N = K, N
    g.lda, g.ldw, g.ldc, g.lds = K, K // 2, N, K // BLOCK
    g.w_expert_stride, g.w_scale_expert_stride = N * (K // 2), N * (K // BLOCK)
    g.n_flat, g.a_div, g.n_experts, g.max_blocks, g.dtype, g.flags = 8, 2, 4, 4, _lib.SLM_BF16, 0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def host_call(g):
    from scalellm_amd import _lib
    return _lib.lib().slm_moe_mxfp4_gemm(C.byref(g), None)


def mxfp4_state_dict(hidden, inter, E, bits, seed=0, gate=True):
    """a Quark-style MoE checkpoint: randn experts (scaled differently per projection and expert) quantised by
    kernels.quantize_mxfp4_weight, uint8 weight / weight_scale under the Mixtral names; the router in T"""
    from scalellm_amd import kernels
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for e in range(E):
        for i, (w, shape) in enumerate((("w1", (inter, hidden)), ("w3", (inter, hidden)), ("w2", (hidden, inter)))):
            p, s = kernels.quantize_mxfp4_weight(torch.randn(*shape, generator=g) / (10 + 3 * i + e))
            sd[f"experts.{e}.{w}.weight"], sd[f"experts.{e}.{w}.weight_scale"] = p, s
    if gate:
        sd["gate.weight"] = (torch.randn(E, hidden, generator=g) * 0.5).to(torch_dtype(bits))
        sd["gate.e_score_correction_bias"] = torch.randn(E, generator=g) * 0.1
    return sd


def dequantized_state_dict(sd, bits):
    """the same checkpoint for unquantised experts: every weight dequantised to T (exact: the scale bytes are asserted
    to be in T's exact range), weight_scale dropped, the router tensors as they are"""
    from scalellm_amd import kernels
    lo, hi = (2, 252) if bits == "bf16" else (114, 140)
    out = {}
    for key, t in sd.items():
        if key.endswith(".weight_scale"):
            assert int(t.min()) >= lo and int(t.max()) <= hi, key
        elif key.endswith(".weight") and key.startswith("experts."):
            out[key] = kernels.dequantize_mxfp4_weight(t, sd[key + "_scale"], torch_dtype(bits))
        else:
            out[key] = t
    return out
