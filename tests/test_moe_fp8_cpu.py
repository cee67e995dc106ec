"""CPU tests of the fp8 grouped GEMM boundary (include/slm_hip.h section 16, slm_moe_fp8_gemm): the exported symbol,
the ctypes mirror of its argument struct, argument validation before any launch, MoEFp8Experts and the layers'
selection without a GPU, and the float64 reference the GPU tests compare against."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from scalellm_amd import _lib

from . import moe_fp8_ref as fref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")

INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -5


def test_slm_moe_fp8_gemm_is_in_the_header_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"SLM_API\s+int\s+slm_moe_fp8_gemm\s*\(const slm_moe_fp8_gemm_args\*", text)
    fn = _lib.lib().slm_moe_fp8_gemm                # AttributeError: not exported
    assert fn.argtypes is not None                  # resolved by _lib with a prototype
    assert fn.argtypes[0]._type_ is _lib.MoeFp8GemmArgs


def test_fp8_gemm_struct_matches_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cname, cls = "slm_moe_fp8_gemm_args", _lib.MoeFp8GemmArgs
    assert [f for f, _ in cls._fields_] == [
        "a", "w", "w_scale", "c", "row_scale", "sorted_token_idxes", "expert_ids", "n_padded_tokens",
        "w_expert_stride", "w_scale_expert_stride", "n_flat", "K", "N", "lda", "ldw", "ldc", "a_div", "n_experts",
        "max_blocks", "dtype", "flags"]
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


K0, N0 = 256, 128


def _gemm(**kw):
    g = _lib.MoeFp8GemmArgs()
    g.a = g.w = g.w_scale = g.c = g.sorted_token_idxes = g.expert_ids = g.n_padded_tokens = 4096   # never touched
    g.K, g.N = K0, N0
    g.lda, g.ldw, g.ldc = K0, K0, N0
    g.w_expert_stride, g.w_scale_expert_stride = N0 * K0, N0
    g.n_flat, g.a_div, g.n_experts, g.max_blocks, g.dtype, g.flags = 8, 2, 4, 4, _lib.SLM_BF16, 0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_fp8_gemm_validation_precedes_any_launch():
    G = _lib.lib().slm_moe_fp8_gemm
    SILU = _lib.SLM_MOE_SILU_MUL
    rc = lambda **kw: G(C.byref(_gemm(**kw)), None)  # noqa: E731
    assert G(None, None) == INVALID
    # null or negative arguments
    for kw in (dict(n_flat=-1), dict(K=0), dict(N=-32), dict(a_div=0), dict(n_experts=0), dict(max_blocks=-1)):
        assert rc(**kw) == INVALID, kw
    for ptr in ("a", "w", "c", "sorted_token_idxes", "expert_ids", "n_padded_tokens"):
        assert rc(**{ptr: None}) == INVALID, ptr
    # unknown flags; SiLU * mul together with a row scale
    assert rc(flags=1) == INVALID
    assert rc(flags=SILU | 4) == INVALID
    assert rc(flags=SILU, ldc=64, row_scale=4096) == INVALID
    # a stride smaller than the extent
    assert rc(lda=248) == INVALID
    assert rc(ldw=240) == INVALID
    assert rc(ldc=120) == INVALID
    assert rc(flags=SILU, ldc=56) == INVALID                                      # SiLU: the extent is N / 2
    assert rc(w_expert_stride=(N0 - 1) * K0 + 240) == INVALID                     # experts would overlap
    assert rc(ldw=K0 + 16, w_expert_stride=N0 * K0) == INVALID                    # ... with a padded row stride too
    assert rc(w_scale_expert_stride=N0 - 1) == INVALID                            # the scales would overlap
    # other dtypes, shapes, size limits
    assert rc(dtype=_lib.SLM_F32) == UNSUPPORTED
    assert rc(K=144, lda=144, ldw=144) == UNSUPPORTED                             # K % 32
    assert rc(N=112, ldc=112) == UNSUPPORTED                                      # N % 32
    assert rc(N=96, ldc=48, flags=SILU) == UNSUPPORTED                            # (N / 2) % 32
    big = 1 << 16
    assert rc(K=big, N=big, lda=big, ldw=big, ldc=big, w_expert_stride=big * big, w_scale_expert_stride=big) \
        == UNSUPPORTED                                                            # one expert of 4 GiB
    assert rc(ldw=1 << 25, w_expert_stride=N0 << 25) == UNSUPPORTED               # N * ldw >= 2^32: through its stride
    assert rc(n_flat=(1 << 31) - 256) == UNSUPPORTED                              # flat indices are int32
    # misaligned pointers or strides (16-byte loads of A and W, fp32 scales)
    assert rc(a=4096 + 8) == ALIGNMENT
    assert rc(w=4096 + 8) == ALIGNMENT
    assert rc(c=4097) == ALIGNMENT
    assert rc(row_scale=4098) == ALIGNMENT
    assert rc(w_scale=4098) == ALIGNMENT
    assert rc(lda=260) == ALIGNMENT
    assert rc(ldw=K0 + 8, w_expert_stride=N0 * (K0 + 8)) == ALIGNMENT             # the stride itself is 16-B aligned
    assert rc(w_expert_stride=N0 * K0 + 8) == ALIGNMENT
    # nothing routed: a no-op, whatever the pointers
    assert rc(n_flat=0, a=None, c=None) == 0
    assert rc(max_blocks=0, w=None, w_scale=None) == 0


# ---- MoEFp8Experts and the layers on "cpu" ----------------------------------------------------------------------------
def _fp8_state_dict(hidden, inter, E, seed=0, scale_form="tensor"):
    """a Mixtral-FP8 style checkpoint: e4m3 weights, and per-tensor scales that DIFFER between w1, w3 and w2 (and
    between experts), in the forms checkpoints use"""
    from scalellm_amd import kernels
    g = torch.Generator().manual_seed(seed)
    sd = {"gate.weight": (torch.randn(E, hidden, generator=g) * 0.5).to(torch.bfloat16)}
    for e in range(E):
        for i, (w, shape) in enumerate((("w1", (inter, hidden)), ("w3", (inter, hidden)), ("w2", (hidden, inter)))):
            w8, s = kernels.quantize_fp8_weight(torch.randn(*shape, generator=g) / (8 + 4 * i + e), scale_form)
            sd[f"experts.{e}.{w}.weight"] = w8
            if scale_form == "tensor":
                s = s[0].clone() if (e + i) % 2 else s[:1].clone()        # 0-d and [1]
            else:
                s = s.view(-1, 1).to(torch.bfloat16) if (e + i) % 2 else s.clone()   # [rows, 1] (bf16) and [rows]
            sd[f"experts.{e}.{w}.weight_scale"] = s
            sd[f"experts.{e}.{w}.input_scale"] = torch.tensor(0.5)       # ignored: W8A16
    return sd


def _bytes(t):
    return t.view(torch.uint8)


@pytest.mark.parametrize("scale_form", ["tensor", "channel"])
def test_fp8_experts_load_verify_and_repack_without_a_gpu(scale_form):
    from scalellm_amd import kernels, moe
    assert callable(kernels.moe_fp8_grouped_gemm)
    H, I, E = 64, 96, 4
    sd = _fp8_state_dict(H, I, E, scale_form=scale_form)
    ex = moe.MoEFp8Experts(H, I, E, torch.bfloat16, "cpu")
    with pytest.raises(AssertionError):
        ex.verify_loaded_weights()                       # nothing loaded yet
    ex.load_state_dict(sd)
    ex.verify_loaded_weights()
    ex.repack()
    assert ex.gate_up.dtype == torch.float8_e4m3fn and ex.down.dtype == torch.float8_e4m3fn
    assert tuple(ex.gate_up.shape) == (E, 2 * I, H) and tuple(ex.down.shape) == (E, H, I)
    assert ex.gate_up.is_contiguous() and ex.down.is_contiguous()
    assert ex.gate_up_scale.dtype == torch.float32 and tuple(ex.gate_up_scale.shape) == (E, 2 * I)
    assert ex.down_scale.dtype == torch.float32 and tuple(ex.down_scale.shape) == (E, H)
    assert ex.gate_up_scale.is_contiguous() and ex.down_scale.is_contiguous()
    flat = lambda key: sd[key].reshape(-1).float()  # noqa: E731
    for e in range(E):                                    # w1 rows, then w3 rows: concatenated, not interleaved
        assert torch.equal(_bytes(ex.gate_up[e, :I]), _bytes(sd[f"experts.{e}.w1.weight"]))
        assert torch.equal(_bytes(ex.gate_up[e, I:]), _bytes(sd[f"experts.{e}.w3.weight"]))
        assert torch.equal(_bytes(ex.down[e]), _bytes(sd[f"experts.{e}.w2.weight"]))
        s1, s3, s2 = (flat(f"experts.{e}.{w}.weight_scale") for w in ("w1", "w3", "w2"))
        if scale_form == "tensor":
            assert float(s1) != float(s3)                 # ... and each half keeps its OWN per-tensor scale
            s1, s3, s2 = s1.expand(I), s3.expand(I), s2.expand(H)
        assert torch.equal(ex.gate_up_scale[e, :I], s1) and torch.equal(ex.gate_up_scale[e, I:], s3)
        assert torch.equal(ex.down_scale[e], s2)
    assert ex.nbytes() == 3 * E * H * I + 4 * E * (2 * I + H)


def test_fp8_experts_reject_what_they_cannot_load():
    from scalellm_amd import moe
    H, I, E = 64, 96, 4
    sd = _fp8_state_dict(H, I, E)
    bad = dict(sd)
    bad["experts.2.w3.weight"] = torch.zeros(I, H, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        moe.MoEFp8Experts(H, I, E, torch.bfloat16, "cpu").load_state_dict(bad)   # nothing is quantised on load
    missing = {k: v for k, v in sd.items() if k != "experts.1.w2.weight_scale"}
    ex = moe.MoEFp8Experts(H, I, E, torch.bfloat16, "cpu")
    ex.load_state_dict(missing)
    with pytest.raises(AssertionError, match=r"experts\.1\.w2\.weight_scale"):
        ex.verify_loaded_weights()
    no_w = {k: v for k, v in sd.items() if k != "experts.0.w3.weight"}
    ex = moe.MoEFp8Experts(H, I, E, torch.bfloat16, "cpu")
    ex.load_state_dict(no_w)
    with pytest.raises(AssertionError, match=r"experts\.0\.w3\.weight is not loaded"):
        ex.verify_loaded_weights()
    wrong = dict(sd)
    wrong["experts.1.w2.weight_scale"] = torch.ones(H + 1)
    ex = moe.MoEFp8Experts(H, I, E, torch.bfloat16, "cpu")
    ex.load_state_dict(wrong)
    with pytest.raises(Exception):
        ex.repack()                                       # neither per tensor nor one per output channel
    swapped = dict(sd)
    swapped["experts.1.w2.weight"] = sd["experts.1.w1.weight"]
    ex = moe.MoEFp8Experts(H, I, E, torch.bfloat16, "cpu")
    ex.load_state_dict(swapped)
    with pytest.raises(Exception):
        ex.repack()                                       # [I, H] where [H, I] belongs
    with pytest.raises(Exception):
        moe.MoEFp8Experts(H, I, E, torch.float32, "cpu")


def test_fp8_experts_expert_offset_selects_the_shard():
    from scalellm_amd import moe
    H, I, E = 64, 96, 4
    sd = _fp8_state_dict(H, I, E)
    ex = moe.MoEFp8Experts(H, I, 2, torch.float16, "cpu", expert_offset=2)
    ex.load_state_dict(sd)
    ex.repack()
    assert tuple(ex.gate_up.shape) == (2, 2 * I, H)
    for e in range(2):
        assert torch.equal(_bytes(ex.gate_up[e, :I]), _bytes(sd[f"experts.{2 + e}.w1.weight"]))
        assert torch.equal(_bytes(ex.down[e]), _bytes(sd[f"experts.{2 + e}.w2.weight"]))
        assert float(ex.down_scale[e, 0]) == float(sd[f"experts.{2 + e}.w2.weight_scale"].reshape(-1)[0])


def test_quant_args_select_the_experts_class():
    from scalellm_amd import moe
    from scalellm_amd.layers import QuantArgs
    H, I, E = 64, 96, 4
    layer = moe.FusedMoE(H, I, E, 2, QuantArgs("fp8", 8), dtype=torch.float16, device="cpu")
    assert isinstance(layer.experts, moe.MoEFp8Experts)
    layer.load_state_dict(_fp8_state_dict(H, I, E))
    layer.experts.verify_loaded_weights()
    assert tuple(layer.gate_weight.shape) == (E, H)
    pg = types.SimpleNamespace(world_size=2, rank=1)
    ep = moe.ExpertParallelMoE(H, I, E, 2, pg, QuantArgs("fp8", 8), device="cpu")
    assert isinstance(ep.experts, moe.MoEFp8Experts)
    assert (ep.experts.n_experts, ep.experts.expert_offset) == (2, 2)
    # the other QuantArgs fields mean nothing to fp8
    assert isinstance(moe.FusedMoE(H, I, E, 2, QuantArgs("fp8", 8, group_size=-1, desc_act=True), device="cpu").experts,
                      moe.MoEFp8Experts)
    with pytest.raises(Exception):
        moe.FusedMoE(H, I, E, 2, QuantArgs("fp8", 4), device="cpu")
    with pytest.raises(Exception):
        moe.ExpertParallelMoE(H, I, E, 2, pg, QuantArgs("fp8", 4), device="cpu")
    with pytest.raises(Exception):
        moe.FusedMoE(80, I, E, 2, QuantArgs("fp8", 8), device="cpu")            # hidden % 32
    with pytest.raises(Exception):
        moe.FusedMoE(H, 80, E, 2, QuantArgs("fp8", 8), device="cpu")            # intermediate % 32
    with pytest.raises(Exception):
        moe.ExpertParallelMoE(80, I, E, 2, pg, QuantArgs("fp8", 8), device="cpu")
    # the other two selections are what they were
    assert isinstance(moe.FusedMoE(H, I, E, 2, quant_args=None, device="cpu").experts, moe.MoEDenseExperts)
    assert isinstance(moe.FusedMoE(256, 384, 8, 2, QuantArgs("awq", 4, 128), device="cpu").experts,
                      moe.MoEQuantExperts)
    assert isinstance(moe.ExpertParallelMoE(H, I, E, 2, pg, device="cpu").experts, moe.MoEDenseExperts)
    assert isinstance(moe.ExpertParallelMoE(256, 384, 8, 2, pg, QuantArgs("gptq", 4, 128), device="cpu").experts,
                      moe.MoEQuantExperts)
    assert "fp8" in QuantArgs.__doc__


# ---- the reference and the case tables --------------------------------------------------------------------------------
def test_grouped_fp8_ref_on_one_flat_index_by_hand():
    # codes 0x38 = 1.0, 0x40 = 2.0, 0xB4 = -0.75, 0x01 = 2^-9 (the smallest subnormal)
    w8 = torch.tensor([[[0x38, 0x40], [0xB4, 0x01]],
                       [[0x40, 0x40], [0x38, 0xB4]]], dtype=torch.uint8)          # [E = 2, N = 2, K = 2]
    assert np.array_equal(fref.w8_as64(w8), fref.e4m3_value(w8.numpy()))          # torch's table = the format's
    a = np.array([[3.0, 5.0], [7.0, 11.0]])
    scale = np.array([[0.5, 4.0], [2.0, 0.25]])
    ids = np.array([[1, 0], [0, 1]], np.int32)                                    # T = 2, k = 2
    out = fref.grouped_fp8_ref(a, w8, scale, ids, 2)
    assert out.shape == (4, 2)
    # flat index 1 = token 0, expert 0: [3 * 1 + 5 * 2, 3 * -0.75 + 5 * 2^-9] * [0.5, 4]
    assert np.array_equal(out[1], [13.0 * 0.5, (-2.25 + 5 * 2.0 ** -9) * 4.0])
    # flat index 3 = token 1, expert 1; with a_div = 1 the same index reads row 3 of a 4-row A
    assert np.array_equal(out[3], [36.0 * 2.0, (7.0 - 8.25) * 0.25])
    a4 = np.vstack([a, a[::-1]])
    assert np.array_equal(fref.grouped_fp8_ref(a4, w8, scale, ids, 1)[3], [(3 + 5) * 2 * 2.0, (3.0 - 3.75) * 0.25])
    assert np.array_equal(fref.grouped_fp8_ref(a, w8, None, ids, 2)[1], [13.0, -2.25 + 5 * 2.0 ** -9])


@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_reference_rounded_once_meets_gemm_tol_and_the_bound_binds(bits):
    """one rounding to T is 2^-9 (bf16) / 2^-12 (f16) relative at worst, about a third of that on average: the
    GEMM_TOL the GPU grid asserts is attainable by a kernel that accumulates in fp32 and rounds once"""
    tol = fref.GEMM_TOL[bits]
    E, k = fref.PROJECT_E, fref.PROJECT_TOPK
    for n, (K, N, T, ad) in enumerate(fref.PROJECT_CASES[::7]):
        rng = np.random.default_rng(n)
        a_div = k if ad == "k" else 1
        a = fref.as64(fref.rounded(rng.standard_normal((T * k // a_div, K)), bits))
        w8, scale = fref.quantized_experts(rng, E, N, K)
        ids = fref.routing(rng, T, k, E, crowd=True)
        want = fref.grouped_fp8_ref(a, w8, fref.as64(scale), ids, a_div)
        assert want.shape == (T * k, N)
        err = fref.rel_err(fref.as64(fref.rounded(want, bits)), want)
        assert 0 < err < tol, (K, N, T, err)
        assert fref.rel_err(want * (1 + 2 * tol), want) > tol            # ... and it does bind


def test_case_tables_cover_every_axis_they_name():
    K, N, E, T, k = fref.SAME_BITS_CASES[0]
    assert fref.EXACT_CASE == fref.SAME_BITS_CASES[0]
    # the launch shapes: NW = 1, 2, 4 (SiLU * mul: 2, 4, 4) over LAUNCH_BLOCKS
    nws = [fref.launch_waves(fref.blocks_of(b, T * k, E), N, False) for b in fref.LAUNCH_BLOCKS]
    assert nws == [1, 2, 4]
    Ks, Ns, Es, Ts, ks = fref.SAME_BITS_SILU
    nws = [fref.launch_waves(fref.blocks_of(b, Ts * ks, Es), Ns, True) for b in fref.LAUNCH_BLOCKS]
    assert set(nws) == {2, 4} and nws[0] == 2
    # chunks: the ring (3) wraps with an odd count; chunks followed by three tail units; T spills into a second block
    assert {c[0] // 128 for c in fref.SAME_BITS_CASES} == {5, 3}
    assert {c[0] % 128 // 32 for c in fref.SAME_BITS_CASES} == {0, 3}
    assert all(c[3] > 32 and c[1] % 128 for c in fref.SAME_BITS_CASES)   # a second block, a part-filled column group
    assert [(K // 128, K % 128 // 32) for K in fref.TAIL_KS] == [(0, 1), (0, 3), (1, 1), (3, 3)]
    # the code sweep with 32 rows still holds every non-NaN code
    codes = np.unique(fref.code_sweep_weight(32, 256).numpy())
    assert codes.size == 254 and 0x7F not in codes and 0xFF not in codes
    assert {c[4] for c in fref.SILU_CASES} == {1, 2, 4} and all((c[1] // 2) % 32 == 0 for c in fref.SILU_CASES)
