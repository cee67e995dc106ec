"""CPU tests of the dense grouped GEMM boundary (include/slm_hip.h section 10, slm_moe_gemm): the exported symbol,
the ctypes mirror of its argument struct, argument validation before any launch, the Python layer without a GPU,
and the numpy reference the GPU tests compare against."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from scalellm_amd import _lib
from scalellm_amd._lib import MoeDenseGemmArgs

from . import moe_dense_ref as dref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")

INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -5


def test_slm_moe_gemm_is_in_the_header_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"SLM_API\s+int\s+slm_moe_gemm\s*\(const slm_moe_gemm_dense_args\*", text)
    assert re.search(r"#define\s+SLM_MOE_SILU_MUL\s+\d+", text)
    fn = _lib.lib().slm_moe_gemm                   # AttributeError: not exported
    assert fn.argtypes is not None                 # resolved by _lib with a prototype
    assert fn.argtypes[0]._type_ is MoeDenseGemmArgs


def test_dense_gemm_struct_matches_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cname, cls = "slm_moe_gemm_dense_args", MoeDenseGemmArgs
    assert [f for f, _ in cls._fields_] == [
        "a", "w", "c", "row_scale", "sorted_token_idxes", "expert_ids", "n_padded_tokens", "w_expert_stride", "n_flat",
        "K", "N", "lda", "ldw", "ldc", "a_div", "n_experts", "max_blocks", "dtype", "flags"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             f'  printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("SILU %d\\n", SLM_MOE_SILU_MUL);', '  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out.pop("size")) == C.sizeof(cls)
    assert int(out.pop("SILU")) == _lib.SLM_MOE_SILU_MUL
    for fname, _ in cls._fields_:
        assert int(out[fname]) == getattr(cls, fname).offset, fname


def _gemm(**kw):
    g = MoeDenseGemmArgs()
    g.a = g.w = g.c = g.sorted_token_idxes = g.expert_ids = g.n_padded_tokens = 4096   # host addresses, never touched
    g.K, g.N = 256, 128
    g.lda, g.ldw, g.ldc = 256, 256, 128
    g.w_expert_stride = 128 * 256
    g.n_flat, g.a_div, g.n_experts, g.max_blocks, g.dtype, g.flags = 8, 2, 4, 4, _lib.SLM_BF16, 0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_dense_gemm_validation_precedes_any_launch():
    G = _lib.lib().slm_moe_gemm
    SILU = _lib.SLM_MOE_SILU_MUL
    assert G(None, None) == INVALID
    # null or negative arguments
    for kw in (dict(n_flat=-1), dict(K=0), dict(N=-32), dict(a_div=0), dict(n_experts=0), dict(max_blocks=-1)):
        assert G(C.byref(_gemm(**kw)), None) == INVALID, kw
    for ptr in ("a", "w", "c", "sorted_token_idxes", "expert_ids", "n_padded_tokens"):
        assert G(C.byref(_gemm(**{ptr: None})), None) == INVALID, ptr
    # unknown flags; SiLU * mul together with a row scale
    assert G(C.byref(_gemm(flags=1)), None) == INVALID
    assert G(C.byref(_gemm(flags=SILU | 4)), None) == INVALID
    assert G(C.byref(_gemm(flags=SILU, ldc=64, row_scale=4096)), None) == INVALID
    # a stride smaller than the extent
    assert G(C.byref(_gemm(lda=248)), None) == INVALID
    assert G(C.byref(_gemm(ldw=248)), None) == INVALID
    assert G(C.byref(_gemm(ldc=120)), None) == INVALID
    assert G(C.byref(_gemm(flags=SILU, ldc=56)), None) == INVALID            # SiLU: the extent is N / 2
    assert G(C.byref(_gemm(w_expert_stride=127 * 256 + 248)), None) == INVALID     # experts would overlap
    assert G(C.byref(_gemm(ldw=264, w_expert_stride=128 * 256)), None) == INVALID  # ... with a padded row stride too
    # other dtypes, shapes, size limits
    assert G(C.byref(_gemm(dtype=_lib.SLM_F32)), None) == UNSUPPORTED
    assert G(C.byref(_gemm(K=144, lda=144, ldw=144)), None) == UNSUPPORTED           # K % 32
    assert G(C.byref(_gemm(N=112, ldc=112)), None) == UNSUPPORTED                    # N % 32
    assert G(C.byref(_gemm(N=96, ldc=48, flags=SILU)), None) == UNSUPPORTED          # (N / 2) % 32
    big = 1 << 16
    assert G(C.byref(_gemm(K=big, N=big // 2, lda=big, ldw=big, ldc=big, w_expert_stride=big * big)), None) \
        == UNSUPPORTED                                                               # one expert of 4 GiB
    assert G(C.byref(_gemm(ldw=1 << 25, w_expert_stride=128 << 25)), None) == UNSUPPORTED   # ... through its stride
    assert G(C.byref(_gemm(n_flat=(1 << 31) - 256)), None) == UNSUPPORTED            # flat indices are int32
    # misaligned pointers or strides (16-byte loads of A and W)
    assert G(C.byref(_gemm(a=4096 + 8)), None) == ALIGNMENT
    assert G(C.byref(_gemm(w=4096 + 2)), None) == ALIGNMENT
    assert G(C.byref(_gemm(c=4097)), None) == ALIGNMENT
    assert G(C.byref(_gemm(row_scale=4098)), None) == ALIGNMENT
    assert G(C.byref(_gemm(lda=260)), None) == ALIGNMENT
    assert G(C.byref(_gemm(ldw=260, w_expert_stride=128 * 260)), None) == ALIGNMENT
    assert G(C.byref(_gemm(w_expert_stride=128 * 256 + 4)), None) == ALIGNMENT
    # nothing routed: a no-op, whatever the pointers
    assert G(C.byref(_gemm(n_flat=0, a=None, c=None)), None) == 0
    assert G(C.byref(_gemm(max_blocks=0, w=None)), None) == 0


def _state_dict(hidden, inter, E, dt, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {"gate.weight": (torch.randn(E, hidden, generator=g) * 0.5).to(dt)}
    for e in range(E):
        sd[f"experts.{e}.w1.weight"] = (torch.randn(inter, hidden, generator=g) / 10).to(dt)
        sd[f"experts.{e}.w3.weight"] = (torch.randn(inter, hidden, generator=g) / 10).to(dt)
        sd[f"experts.{e}.w2.weight"] = (torch.randn(hidden, inter, generator=g) / 10).to(dt)
    return sd


def test_dense_experts_construct_and_load_without_a_gpu():
    from scalellm_amd import kernels, moe
    from scalellm_amd.layers import QuantArgs
    assert callable(kernels.moe_grouped_gemm)
    H, I, E = 64, 96, 4
    sd = _state_dict(H, I, E, torch.bfloat16)
    ex = moe.MoEDenseExperts(H, I, E, torch.bfloat16, "cpu")
    with pytest.raises(AssertionError):
        ex.verify_loaded_weights()                       # nothing loaded yet
    ex.load_state_dict(sd)
    ex.verify_loaded_weights()
    ex.repack()
    assert tuple(ex.gate_up.shape) == (E, 2 * I, H) and tuple(ex.down.shape) == (E, H, I)
    assert ex.gate_up.is_contiguous() and ex.down.is_contiguous()
    for e in range(E):                                    # w1 rows, then w3 rows: concatenated, not interleaved
        assert torch.equal(ex.gate_up[e, :I], sd[f"experts.{e}.w1.weight"])
        assert torch.equal(ex.gate_up[e, I:], sd[f"experts.{e}.w3.weight"])
        assert torch.equal(ex.down[e], sd[f"experts.{e}.w2.weight"])
    assert ex.nbytes() == 3 * E * H * I * 2
    bad = dict(sd)
    bad["experts.1.w2.weight"] = bad["experts.1.w2.weight"].t().contiguous()
    ex2 = moe.MoEDenseExperts(H, I, E, torch.bfloat16, "cpu")
    ex2.load_state_dict(bad)
    with pytest.raises(Exception):
        ex2.repack()                                      # [in, out] instead of [out, in]
    with pytest.raises(Exception):
        moe.MoEDenseExperts(H, I, E, torch.float32, "cpu")

    layer = moe.FusedMoE(H, I, E, 2, quant_args=None, dtype=torch.float16, device="cpu")
    assert isinstance(layer.experts, moe.MoEDenseExperts)
    layer.load_state_dict(_state_dict(H, I, E, torch.float16))
    layer.experts.verify_loaded_weights()
    assert tuple(layer.gate_weight.shape) == (E, H)
    assert isinstance(moe.FusedMoE(H, I, E, 2, dtype=torch.float16, device="cpu").experts, moe.MoEDenseExperts)
    with pytest.raises(Exception):
        moe.FusedMoE(80, I, E, 2, quant_args=None, device="cpu")            # hidden % 32
    # with a QuantArgs nothing changes
    q = moe.FusedMoE(256, 384, 8, 2, QuantArgs("awq", 4, 128), device="cpu")
    assert isinstance(q.experts, moe.MoEQuantExperts)
    with pytest.raises(Exception):
        moe.FusedMoE(64, 96, 4, 2, QuantArgs("awq", 4, 32), device="cpu")  # int4: multiples of 128


def test_case_lists_cover_every_axis():
    assert 40 <= len(dref.REF_CASES) <= 55            # x 2 dtypes: about 100 cases
    for axis, want in enumerate(dref.REF_AXES):
        assert {c[axis] for c in dref.REF_CASES} == set(want), axis
    for axis, want in enumerate(dref.PROJECT_AXES):
        assert {c[axis] for c in dref.PROJECT_CASES} == set(want), axis


@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_reference_meets_the_reference_bounds_against_itself(bits):
    """fp64 matmul over dtype-rounded randn / 10 inputs, rounded once to the dtype, passes the reference test's own
    allclose against the unrounded fp64 result: the bounds the GPU grid asserts are attainable by any kernel that
    accumulates in fp32 and rounds once (2^-9 / 2^-12 relative against rtol = 1e-2 / 1e-3)."""
    tol = dref.REF_ALLCLOSE[bits]
    for n, (m, N, K, E, topk) in enumerate(dref.REF_CASES):
        rng = np.random.default_rng(n)
        a = dref.as64(dref.rounded(rng.standard_normal((m, K)) / 10, bits))
        w = dref.as64(dref.rounded(rng.standard_normal((E, N, K)) / 10, bits))
        ids = dref.routing(rng, m, topk, E)
        want = dref.grouped_ref(a, w, ids, topk)
        assert want.shape == (m * topk, N)
        f = m * topk - 1                                  # the last flat index by hand
        np.testing.assert_allclose(want[f], w[ids.reshape(-1)[f]] @ a[f // topk], rtol=1e-12, atol=1e-15)
        assert dref.allclose(dref.as64(dref.rounded(want, bits)), want, tol), (m, N, K, E, topk)
        assert not dref.allclose(want + 2 * tol * (1 + np.abs(want).max()), want, tol)   # ... and they do bind
