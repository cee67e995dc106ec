"""CPU tests of the mixture-of-experts boundary (include/slm_hip.h section 10): exported symbols, the ctypes
mirrors of the argument structs, the numpy oracle against hand-worked cases of every contract, the capacity
bound, and argument validation before any launch."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from scalellm_amd import _lib
from scalellm_amd._lib import MoeAlignArgs, MoeGemmArgs

from . import moe_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")

INVALID, UNSUPPORTED = -1, -2


def test_every_moe_symbol_of_the_header_is_exported_and_bound():
    names = sorted(set(re.findall(r"SLM_API\s+\w+\s+(slm_moe_\w+)\(", open(HEADER).read())))
    assert names == ["slm_moe_align_block", "slm_moe_align_capacity", "slm_moe_grouped_topk_sigmoid",
                     "slm_moe_sum", "slm_moe_topk_softmax", "slm_moe_w4a16_gemm"]
    L = _lib.lib()
    for n in names:
        fn = getattr(L, n)                      # AttributeError: not exported
        assert fn.argtypes is not None, n        # resolved by _lib with a prototype


@pytest.mark.parametrize("cname,cls", [("slm_moe_align_args", MoeAlignArgs), ("slm_moe_gemm_args", MoeGemmArgs)])
def test_moe_structs_match_the_c_header(tmp_path, cname, cls):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             f'  printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("SILU %d\\n", SLM_W4_SILU_MUL);', '  printf("PAIRED %d\\n", SLM_W4_PAIRED);', '  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out.pop("size")) == C.sizeof(cls)
    assert int(out.pop("SILU")) == _lib.SLM_W4_SILU_MUL and int(out.pop("PAIRED")) == _lib.SLM_W4_PAIRED
    for fname, _ in cls._fields_:
        assert int(out[fname]) == getattr(cls, fname).offset, fname


# ---- the oracle against hand-worked cases ----------------------------------------------------------
def test_oracle_topk_softmax_ties_and_renormalize():
    x = np.array([[1.0, 3.0, 3.0, 2.0], [0.0, -0.0, -1.0, -1.0]], np.float32)
    w, i = ref.topk_softmax(x, 2)
    assert i.tolist() == [[1, 2], [0, 1]]             # equal logits (and -0 == +0): the lower index first
    e = np.exp(np.array([1.0, 3.0, 3.0, 2.0]) - 3.0)
    np.testing.assert_allclose(w[0], [e[1] / e.sum(), e[2] / e.sum()], rtol=1e-15)
    assert w[0].sum() < 1.0                           # softmax over ALL experts: the k weights do not sum to 1
    wr, ir = ref.topk_softmax(x, 2, renormalize=True)
    assert ir.tolist() == i.tolist()
    np.testing.assert_allclose(wr[0], [0.5, 0.5], rtol=1e-15)
    np.testing.assert_allclose(wr.sum(axis=1), 1.0, rtol=1e-15)
    w3, i3 = ref.topk_softmax(np.log(np.array([[1.0, 2.0, 4.0, 1.0]])), 3)
    assert i3.tolist() == [[2, 1, 0]]                 # descending; the tie 0 / 3 goes to 0
    np.testing.assert_allclose(w3[0], [0.5, 0.25, 0.125], rtol=1e-12)


def test_oracle_grouped_sigmoid_group_selection_and_unbiased_weights():
    # 8 experts, 4 groups of 2; sigmoid(0) = .5 everywhere, the bias alone decides
    x = np.zeros((1, 8))
    bias = np.array([0.375, -0.5,   0.125, 0.125,   0.25, 0.0,   0.0, 0.0625])   # exact in binary
    # group scores (top-2 sum = both members): 0.875, 1.25, 1.25, 1.0625 -> groups 1 and 2 (the single best expert,
    # 0 in group 0, is NOT selected: its group loses on the top-2 sum)
    w, i, m = ref.grouped_topk_sigmoid(x, bias, 4, 2, 3, 2.5, with_margin=True)
    assert i.tolist() == [[4, 2, 3]]                  # c: .75 (4), .625 (2), .625 (3: tie, the lower index)
    np.testing.assert_allclose(w, 0.5 * 2.5)          # the unbiased sigmoid times the scaling factor
    assert m[0] == pytest.approx(0.0, abs=1e-12)      # the 2 / 3 tie: a zero margin
    # group tie 1.25 / 1.25 with topk_group = 1: the lower group wins
    _, i1 = ref.grouped_topk_sigmoid(x, bias, 4, 1, 2, 1.0)
    assert i1.tolist() == [[2, 3]]
    # a clear case has a positive margin: the smallest gap among group cut and candidates
    bias2 = np.array([0.375, 0.25,   0.0, 0.0,   0.125, 0.0625,   -0.25, -0.25])
    _, i2, m2 = ref.grouped_topk_sigmoid(x, bias2, 4, 2, 2, 1.0, with_margin=True)
    assert i2.tolist() == [[0, 1]]
    assert m2[0] == 0.125                             # candidates .875, .75, .625; group cut 1.1875 vs 1.0
    xs = np.array([[2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    w3, i3 = ref.grouped_topk_sigmoid(xs, np.zeros(8), 4, 1, 1, 1.0)
    assert i3.tolist() == [[0]] and w3[0, 0] == pytest.approx(1 / (1 + np.exp(-2.0)))


def test_oracle_align_block_layout():
    ids = np.array([[2, 0], [2, 3], [0, 2]], np.int32)       # T = 3, k = 2, n_flat = 6; expert 1 is empty
    s, e, n, cu = ref.align_block(ids, 4, 4)
    assert n == 12 and e.tolist() == [0, 2, 3]               # an empty expert gets no block
    assert s.tolist() == [1, 4, 6, 6,  0, 2, 5, 6,  3, 6, 6, 6]   # ascending inside an expert; padding id T * k
    assert cu.tolist() == [0, 4, 4, 8, 12]
    s, e, n, _ = ref.align_block(np.array([[1], [1], [1], [1], [1]], np.int32), 2, 2)
    assert s.tolist() == [0, 1, 2, 3, 4, 5] and e.tolist() == [1, 1, 1] and n == 6
    s, e, n, _ = ref.align_block(np.zeros((0, 2), np.int32), 4, 16)
    assert n == 0 and s.size == 0 and e.size == 0


ADVERSARIAL = [(1, 1, 8), (1, 2, 64), (3, 2, 8), (5, 8, 256), (33, 2, 8), (64, 1, 64), (256, 8, 8), (1024, 2, 1024),
               (7, 8, 64)]


@pytest.mark.parametrize("block", [16, 32, 64, 128, 256])
def test_align_capacity_bounds_adversarial_assignments(block):
    L = _lib.lib()
    for T, k, E in ADVERSARIAL:
        mp, mb = C.c_int64(), C.c_int64()
        assert L.slm_moe_align_capacity(T * k, E, block, C.byref(mp), C.byref(mb)) == 0
        assert (mp.value, mb.value) == ref.align_capacity(T * k, E, block)
        assert mp.value == mb.value * block
        assert mp.value <= T * k + E * (block - 1)            # never looser than the reference test's bound
        worst = 0
        for ids in ref.adversarial_assignments(T, k, E).values():
            _, e, n, _ = ref.align_block(ids, E, block)
            assert n <= mp.value and e.size <= mb.value
            worst = max(worst, n)
        if T * k <= E:                                         # T * k < E: one entry per expert is the worst case
            assert worst == T * k * block == mp.value          # ... and the bound is tight
    assert L.slm_moe_align_capacity(10, 8, 0, None, None) == INVALID
    assert L.slm_moe_align_capacity(10, 8, 48, None, None) == INVALID
    assert L.slm_moe_align_capacity(10, 1025, 32, None, None) == INVALID
    assert L.slm_moe_align_capacity(-1, 8, 32, None, None) == INVALID


# ---- validation before any launch: null / host pointers never reach a kernel -------------------------
def test_routing_validation_precedes_any_launch():
    L = _lib.lib()
    S, G = L.slm_moe_topk_softmax, L.slm_moe_grouped_topk_sigmoid
    P = 4096                                                 # a host address no kernel may touch
    assert S(P, P, P, 4, 6, 2, 0, None) == UNSUPPORTED       # E not a power of two
    assert S(P, P, P, 4, 512, 2, 0, None) == UNSUPPORTED     # E > 256
    assert S(P, P, P, 4, 8, 9, 0, None) == INVALID           # k > E
    assert S(P, P, P, 4, 8, 0, 0, None) == INVALID           # k < 1
    assert S(None, P, P, 4, 8, 2, 0, None) == INVALID
    assert S(None, None, None, 0, 8, 2, 0, None) == 0        # no tokens: a no-op
    assert G(P, P, P, P, 4, 24, 8, 4, 2, 1.0, None) == UNSUPPORTED       # E not a power of two
    assert G(P, P, P, P, 4, 16, 8, 4, 17, 1.0, None) == INVALID          # k > E
    assert G(P, P, P, P, 4, 16, 3, 2, 2, 1.0, None) == INVALID           # groups do not divide E
    assert G(P, P, P, P, 4, 16, 16, 4, 2, 1.0, None) == INVALID          # groups of one expert: no top-2
    assert G(P, P, P, P, 4, 16, 8, 9, 2, 1.0, None) == INVALID           # topk_group > groups
    assert G(P, P, P, P, 4, 16, 8, 2, 5, 1.0, None) == INVALID           # k > experts in the kept groups
    assert G(P, None, P, P, 4, 16, 8, 2, 2, 1.0, None) == INVALID        # no bias


def _align(**kw):
    a = MoeAlignArgs()
    a.topk_ids = a.sorted_token_idxes = a.expert_ids = a.n_padded_tokens = 4096
    a.n_flat, a.n_experts, a.block_size = 16, 8, 32
    a.sorted_capacity, a.blocks_capacity = ref.align_capacity(16, 8, 32)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_align_and_sum_validation_precedes_any_launch():
    L = _lib.lib()
    A = L.slm_moe_align_block
    assert A(None, None) == INVALID
    assert A(C.byref(_align(block_size=0)), None) == INVALID
    assert A(C.byref(_align(block_size=24)), None) == INVALID
    assert A(C.byref(_align(n_experts=0)), None) == INVALID
    assert A(C.byref(_align(n_experts=2048)), None) == INVALID
    assert A(C.byref(_align(sorted_token_idxes=None)), None) == INVALID
    assert A(C.byref(_align(sorted_capacity=255)), None) == INVALID      # below the capacity rule (8 * 32)
    assert A(C.byref(_align(blocks_capacity=7)), None) == INVALID
    M = L.slm_moe_sum
    assert M(4096, 4096, 4, 0, 64, 1, None) == INVALID                   # k < 1
    assert M(4096, 4096, 4, 2, 64, 2, None) == UNSUPPORTED               # fp32 is not an activation dtype
    assert M(None, 4096, 4, 2, 64, 1, None) == INVALID
    assert M(None, None, 0, 2, 64, 1, None) == 0


def _gemm(**kw):
    g = MoeGemmArgs()
    g.a = g.wq = g.sz = g.c = g.sorted_token_idxes = g.expert_ids = g.n_padded_tokens = 4096
    g.K, g.N, g.group_size = 256, 128, 128
    g.wq_expert_stride, g.sz_expert_stride = 256 * 128 // 2, 2 * 128 * 4
    g.n_flat, g.lda, g.ldc = 8, 256, 128
    g.a_div, g.n_experts, g.max_blocks, g.dtype, g.format, g.flags = 2, 4, 4, _lib.SLM_BF16, _lib.SLM_W4_AWQ, 0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_grouped_gemm_validation_precedes_any_launch():
    L = _lib.lib()
    G = L.slm_moe_w4a16_gemm
    assert G(None, None) == INVALID
    assert G(C.byref(_gemm(K=192, lda=192, group_size=64)), None) == UNSUPPORTED     # K % 128 != 0
    assert G(C.byref(_gemm(N=96, ldc=96)), None) == UNSUPPORTED                      # N % 64 != 0
    assert G(C.byref(_gemm(perm=4096)), None) == UNSUPPORTED                         # act-order experts
    assert G(C.byref(_gemm(bias=4096)), None) == UNSUPPORTED
    paired = _lib.SLM_W4_AWQ | _lib.SLM_W4_PAIRED
    assert G(C.byref(_gemm(N=96, ldc=48, flags=_lib.SLM_W4_SILU_MUL, format=paired)), None) == UNSUPPORTED
    assert G(C.byref(_gemm(flags=_lib.SLM_W4_SILU_MUL)), None) == INVALID            # SiLU on unpaired experts
    assert G(C.byref(_gemm(flags=_lib.SLM_W4_SILU_MUL, format=paired, row_scale=4096)), None) == INVALID
    assert G(C.byref(_gemm(format=_lib.SLM_W8_GPTQ)), None) == UNSUPPORTED           # 8-bit planes
    assert G(C.byref(_gemm(format=_lib.SLM_W8_AWQ)), None) == UNSUPPORTED
    assert G(C.byref(_gemm(dtype=_lib.SLM_F32)), None) == UNSUPPORTED
    assert G(C.byref(_gemm(group_size=48)), None) == UNSUPPORTED
    assert G(C.byref(_gemm(flags=_lib.SLM_W4_DEFER_REDUCE)), None) == INVALID        # no split-K here
    assert G(C.byref(_gemm(a_div=0)), None) == INVALID
    assert G(C.byref(_gemm(expert_ids=None)), None) == INVALID
    assert G(C.byref(_gemm(wq_expert_stride=100)), None) == INVALID                  # experts would overlap
    assert G(C.byref(_gemm(ldc=64)), None) == -5                                     # ldc < N
    assert G(C.byref(_gemm(n_flat=0, a=None, c=None)), None) == 0                    # nothing routed: a no-op


def test_python_layer_exists_without_a_gpu():
    from scalellm_amd import kernels, moe
    from scalellm_amd.layers import QuantArgs
    assert kernels.MOE_GEMM_BLOCK == 32
    assert kernels.moe_align_capacity(3, 8, 32) == (96, 3)
    with pytest.raises(Exception):
        moe.FusedMoE(256, 384, 8, 9, QuantArgs("awq", 4, 128), device="cpu")      # topk > n_experts
    with pytest.raises(Exception):
        moe.FusedMoE(256, 384, 8, 2, QuantArgs("gptq", 8, 128), device="cpu")      # 8-bit experts
