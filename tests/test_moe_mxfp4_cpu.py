"""CPU tests of the MXFP4 grouped GEMM boundary (include/slm_hip.h section 21, slm_moe_mxfp4_gemm): the exported
symbol, the ctypes mirror of its argument struct, argument validation before any launch (stand-in pointers, never
dereferenced), MoEMxfp4Experts and the layers' selection without a GPU, and the float64 reference the GPU tests
compare against."""
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

from . import moe_mxfp4_ref as mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")

INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -5


def test_slm_moe_mxfp4_gemm_is_in_the_header_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"SLM_API\s+int\s+slm_moe_mxfp4_gemm\s*\(const slm_moe_mxfp4_gemm_args\*", text)
    assert re.search(r"/\* 21\. MXFP4 mixture-of-experts", text)
    fn = _lib.lib().slm_moe_mxfp4_gemm              # AttributeError: not exported
    assert fn.argtypes is not None                  # resolved by _lib with a prototype
    assert fn.argtypes[0]._type_ is _lib.MoeMxfp4GemmArgs


def test_mxfp4_gemm_struct_matches_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cname, cls = "slm_moe_mxfp4_gemm_args", _lib.MoeMxfp4GemmArgs
    names = [f for f, _ in cls._fields_]
    assert names == [f for f, _ in _lib.MoeFp8GemmArgs._fields_] + ["lds"]    # section 16's block, plus the row stride
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             f'  printf("size %zu\\n", sizeof({cname}));']
    for fname in names:
        lines.append(f'  printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out.pop("size")) == C.sizeof(cls)
    for fname in names:
        assert int(out[fname]) == getattr(cls, fname).offset, fname


K0, N0 = 256, 128
KB, KS = K0 // 2, K0 // 32        # bytes of a weight row, of a scale row


def test_mxfp4_gemm_validation_precedes_any_launch():
    SILU = _lib.SLM_MOE_SILU_MUL
    rc = lambda **kw: mx.host_call(mx.host_args(K0, N0, **kw))  # noqa: E731
    assert _lib.lib().slm_moe_mxfp4_gemm(None, None) == INVALID
    # null or negative arguments
    for kw in (dict(n_flat=-1), dict(K=0), dict(N=-32), dict(a_div=0), dict(n_experts=0), dict(max_blocks=-1)):
        assert rc(**kw) == INVALID, kw
    for ptr in ("a", "w", "c", "sorted_token_idxes", "expert_ids", "n_padded_tokens"):
        assert rc(**{ptr: None}) == INVALID, ptr
    assert rc(w_scale=None) == INVALID                                            # the block scales are required
    # unknown flags; SiLU * mul together with a row scale
    assert rc(flags=1) == INVALID
    assert rc(flags=SILU | 4) == INVALID
    assert rc(flags=SILU, ldc=64, row_scale=4096) == INVALID
    # a stride smaller than the extent
    assert rc(lda=248) == INVALID
    assert rc(ldw=KB - 16) == INVALID                                             # ldw counts bytes: K / 2
    assert rc(ldw=K0 // 4) == INVALID
    assert rc(ldc=120) == INVALID
    assert rc(flags=SILU, ldc=56) == INVALID                                      # SiLU: the extent is N / 2
    assert rc(w_expert_stride=(N0 - 1) * KB + KB - 16) == INVALID                 # experts would overlap
    assert rc(ldw=KB + 16, w_expert_stride=N0 * KB) == INVALID                    # ... with a padded row stride too
    assert rc(lds=KS - 1) == INVALID                                              # a scale row shorter than K / 32
    assert rc(w_scale_expert_stride=(N0 - 1) * KS + KS - 1) == INVALID            # the scales would overlap
    assert rc(lds=KS + 3, w_scale_expert_stride=N0 * KS) == INVALID               # ... with a padded row stride too
    # other dtypes, shapes, size limits
    assert rc(dtype=_lib.SLM_F32) == UNSUPPORTED
    assert rc(K=144, lda=144, ldw=80, lds=5) == UNSUPPORTED                       # K % 32
    assert rc(N=112, ldc=112) == UNSUPPORTED                                      # N % 32
    assert rc(N=96, ldc=48, flags=SILU) == UNSUPPORTED                            # (N / 2) % 32
    big = 1 << 17
    assert rc(K=big, N=big, lda=big, ldw=big // 2, ldc=big, lds=big // 32, w_expert_stride=big * big // 2,
              w_scale_expert_stride=big * big // 32) == UNSUPPORTED               # one expert of 8 GiB
    assert rc(ldw=1 << 25, w_expert_stride=N0 << 25) == UNSUPPORTED               # N * ldw >= 2^32: through its stride
    assert rc(lds=1 << 25, w_scale_expert_stride=N0 << 25) == UNSUPPORTED         # N * lds >= 2^32
    assert rc(n_flat=(1 << 31) - 256) == UNSUPPORTED                              # flat indices are int32
    # misaligned pointers or strides (16-byte loads of A and W)
    assert rc(a=4096 + 8) == ALIGNMENT
    assert rc(w=4096 + 8) == ALIGNMENT
    assert rc(c=4097) == ALIGNMENT
    assert rc(row_scale=4098) == ALIGNMENT
    assert rc(lda=260) == ALIGNMENT
    assert rc(ldw=KB + 8, w_expert_stride=N0 * (KB + 8)) == ALIGNMENT             # ldw % 16
    assert rc(w_expert_stride=N0 * KB + 8) == ALIGNMENT                           # w_expert_stride % 16
    # nothing routed: a no-op, whatever the pointers
    assert rc(n_flat=0, a=None, c=None) == 0
    assert rc(n_flat=0, w_scale=None) == 0
    assert rc(max_blocks=0, w=None, w_scale=None) == 0


def test_the_scale_side_carries_no_alignment_requirement():
    """K = 672: a scale row of 21 bytes.  With stand-in pointers no call here may get as far as a launch, so an odd
    scale base, row stride and expert stride are shown to pass by the rule that fails AFTER them: the block is
    refused for its weight base (SLM_ERR_ALIGNMENT comes after every SLM_ERR_INVALID_ARG check), not for its scales"""
    K, N = 672, 64
    assert mx.host_call(mx.host_args(K, N, n_flat=0)) == 0
    g = mx.host_args(K, N, w_scale=4097, lds=23, w_scale_expert_stride=(N - 1) * 23 + 21, w=4096 + 8)
    assert mx.host_call(g) == ALIGNMENT                                           # the weight base, not the scales
    g = mx.host_args(K, N, w_scale=4097, lds=23, w_scale_expert_stride=(N - 1) * 23 + 20)
    assert mx.host_call(g) == INVALID                                             # one byte short of the last row
    g = mx.host_args(K, N, w_scale=4097, lds=20)
    assert mx.host_call(g) == INVALID


# ---- the reference --------------------------------------------------------------------------------------------------------
def test_grouped_mxfp4_ref_on_two_experts_by_hand():
    # codes: 2 = 1.0, 7 = 6.0, 0xB = -1.5, 1 = 0.5; a byte's LOW nibble is the lower k
    K, N, E = 32, 2, 2
    codes = np.zeros((E, N, K), np.int64)
    codes[0, 0, 0], codes[0, 0, 1], codes[0, 1, 31] = 2, 7, 0xB       # expert 0: row 0 = [1, 6, 0...], row 1 = [... -1.5]
    codes[1, 0, 0], codes[1, 0, 1], codes[1, 1, 30] = 7, 2, 1         # expert 1: row 0 = [6, 1, 0...], row 1 = [.. .5, 0]
    packed = torch.stack([mx.mref.pack(codes[e]) for e in range(E)])
    assert packed[0, 0, 0] == 0x72 and packed[0, 1, 15] == 0xB0 and packed[1, 1, 15] == 0x01
    scale = torch.tensor([[[128], [126]], [[127], [130]]], dtype=torch.uint8)     # 2, 1/2; 1, 8
    w = mx.experts_as64(packed, scale)
    assert w.shape == (E, N, K)
    assert list(w[0, 0, :3]) == [2.0, 12.0, 0.0] and w[0, 1, 31] == -0.75
    assert list(w[1, 0, :3]) == [6.0, 1.0, 0.0] and w[1, 1, 30] == 4.0
    a = np.zeros((2, K))
    a[0, 0], a[0, 1], a[0, 30], a[0, 31] = 3.0, 5.0, 7.0, 11.0
    a[1, 0], a[1, 1], a[1, 30], a[1, 31] = 1.0, -1.0, 2.0, 4.0
    ids = np.array([[1, 0], [0, 1]], np.int32)                        # T = 2, k = 2
    out = mx.grouped_mxfp4_ref(a, packed, scale, ids, 2)
    assert out.shape == (4, 2)
    assert np.array_equal(out[0], [3 * 6.0 + 5 * 1.0, 7 * 4.0])       # token 0, expert 1
    assert np.array_equal(out[1], [3 * 2.0 + 5 * 12.0, 11 * -0.75])   # token 0, expert 0
    assert np.array_equal(out[2], [1 * 2.0 - 12.0, 4 * -0.75])        # token 1, expert 0
    assert np.array_equal(out[3], [6.0 - 1.0, 2 * 4.0])               # token 1, expert 1
    # a_div = 1: flat index f reads row f of a 4-row A
    a4 = np.vstack([a, a[::-1]])
    assert np.array_equal(mx.grouped_mxfp4_ref(a4, packed, scale, ids, 1)[3], [3 * 6.0 + 5 * 1.0, 7 * 4.0])


def test_generators_and_case_tables_cover_what_they_name():
    rng = np.random.default_rng(0)
    p, s = mx.random_experts(rng, 8, 160, 672)
    assert tuple(p.shape) == (8, 160, 336) and tuple(s.shape) == (8, 160, 21)
    assert int(s.min()) == 118 and int(s.max()) == 126
    assert np.unique(mx.mref.unpack(p[0])).size == 16                  # every code
    for bits in ("bf16", "f16"):                                       # ... all exact in both dtypes
        w = mx.experts_as64(p[:1, :8], s[:1, :8])
        assert np.array_equal(mx.as64(mx.rounded(w, bits)), w)
    # chunks and tail units of the K list
    assert [(K // 128, K % 128 // 32) for K in mx.SAME_BITS_KS] == [(0, 3), (1, 0), (1, 1), (3, 1), (5, 1)]
    assert 672 // 32 == 21
    # the launch shapes each N reaches
    n_flat, E = mx.SAME_BITS_T * mx.SAME_BITS_TOPK, mx.SAME_BITS_E
    nw = lambda N, b, silu: mx.launch_waves(mx.blocks_of(b, n_flat, E), N, silu)  # noqa: E731
    assert [nw(160, b, False) for b in mx.LAUNCH_BLOCKS[160]] == [1, 2, 4]
    assert [nw(32, b, False) for b in mx.LAUNCH_BLOCKS[32]] == [1, 4]
    assert [nw(64, b, False) for b in mx.LAUNCH_BLOCKS[64]] == [1, 4]
    assert [nw(64, b, True) for b in mx.SILU_BLOCKS[64]] == [2, 4]
    assert [nw(192, b, True) for b in mx.SILU_BLOCKS[192]] == [2, 2, 4]
    assert set(mx.LAUNCH_BLOCKS) == set(mx.SAME_BITS_NS)
    # the scale pattern: neighbours in e, n and b never share a byte, and both ranges are exact in their dtype
    for bits, lo, hi in (("bf16", 100, 200), ("f16", 114, 140)):
        s = mx.scale_pattern(8, 64, 5, bits).numpy().astype(np.int64)
        assert s.min() >= lo and s.max() <= hi
        assert s[-1, -1, -1] == lo + (37 * 7 + 5 * 63 + 4) % (hi - lo + 1)
        for b in range(5):
            for b2 in range(5):
                assert not (s[:, :-1, b] == s[:, 1:, b2]).any() and not (s[:-1, :, b] == s[1:, :, b2]).any()
                assert b == b2 or not (s[:, :, b] == s[:, :, b2]).any()
    # the code sweep: the expert id offsets the code and the scale
    p, s = mx.code_sweep_experts(2, 32, 160)
    c0, c1 = mx.mref.unpack(p[0]), mx.mref.unpack(p[1])
    assert c0[3, 5] == 8 and c1[3, 5] == 9 and np.array_equal((c0 + 1) % 16, c1)
    assert int(s[0, 0, 0]) == 114 and int(s[1, 0, 0]) == 115
    # small integers: exact inputs
    a, p, s = mx.int_experts(rng, 4, 10, 160, 32)
    assert a.shape == (10, 160) and tuple(p.shape) == (4, 32, 80) and tuple(s.shape) == (4, 32, 5)
    w = mx.experts_as64(p, s)
    assert np.array_equal(w * 4, np.round(w * 4)) and np.abs(w).max() <= 12


# ---- MoEMxfp4Experts and the layers on "cpu" -----------------------------------------------------------------------------
H, I, E = 64, 96, 4


def test_mxfp4_experts_load_verify_and_repack_without_a_gpu():
    from scalellm_amd import kernels, moe
    assert callable(kernels.moe_mxfp4_grouped_gemm)
    sd = mx.mxfp4_state_dict(H, I, E, "bf16")
    ex = moe.MoEMxfp4Experts(H, I, E, torch.bfloat16, "cpu")
    with pytest.raises(AssertionError):
        ex.verify_loaded_weights()                       # nothing loaded yet
    ex.load_state_dict(sd)
    ex.verify_loaded_weights()
    ex.repack()
    for t in (ex.gate_up, ex.down, ex.gate_up_scale, ex.down_scale):
        assert t.dtype == torch.uint8 and t.is_contiguous()
    assert tuple(ex.gate_up.shape) == (E, 2 * I, H // 2) and tuple(ex.gate_up_scale.shape) == (E, 2 * I, H // 32)
    assert tuple(ex.down.shape) == (E, H, I // 2) and tuple(ex.down_scale.shape) == (E, H, I // 32)
    for e in range(E):                                    # w1 rows, then w3 rows: concatenated, not interleaved
        for name, t in (("weight", ex.gate_up), ("weight_scale", ex.gate_up_scale)):
            assert torch.equal(t[e, :I], sd[f"experts.{e}.w1.{name}"])
            assert torch.equal(t[e, I:], sd[f"experts.{e}.w3.{name}"])
        assert not torch.equal(ex.gate_up[e, :I], ex.gate_up[e, I:])
        assert torch.equal(ex.down[e], sd[f"experts.{e}.w2.weight"])
        assert torch.equal(ex.down_scale[e], sd[f"experts.{e}.w2.weight_scale"])
    assert ex.nbytes() == 3 * E * H * I // 2 + 3 * E * H * I // 32       # 4.25 bits a weight
    # typed views of the same bytes and the blocked [rows, K/32, 16] form load to the same tensors
    typed = dict(sd)
    if hasattr(torch, "float8_e8m0fnu"):
        typed["experts.1.w2.weight_scale"] = sd["experts.1.w2.weight_scale"].view(torch.float8_e8m0fnu)
    typed["experts.2.w1.weight"] = sd["experts.2.w1.weight"].view(I, H // 32, 16)
    ex2 = moe.MoEMxfp4Experts(H, I, E, torch.float16, "cpu")
    ex2.load_state_dict(typed)
    ex2.repack()
    assert torch.equal(ex2.gate_up, ex.gate_up) and torch.equal(ex2.down_scale, ex.down_scale)
    assert ex2.down_scale.dtype == torch.uint8


def test_mxfp4_experts_reject_what_they_cannot_load():
    from scalellm_amd import moe
    from scalellm_amd.kernels import SlmError
    sd = mx.mxfp4_state_dict(H, I, E, "bf16")
    new = lambda: moe.MoEMxfp4Experts(H, I, E, torch.bfloat16, "cpu")  # noqa: E731
    for key, t in (("experts.2.w3.weight", torch.zeros(I, H, dtype=torch.bfloat16)),         # nothing is quantised
                   ("experts.2.w3.weight", torch.zeros(I, H // 2, dtype=torch.int8)),
                   ("experts.0.w2.weight_scale", torch.ones(H, I // 32)),                    # a float scale
                   ("experts.0.w2.weight_scale", torch.ones(H, I // 32, dtype=torch.int32))):
        bad = dict(sd)
        bad[key] = t
        with pytest.raises(TypeError):
            new().load_state_dict(bad)
    for missing_key in ("experts.1.w2.weight_scale", "experts.0.w3.weight"):
        ex = new()
        ex.load_state_dict({k: v for k, v in sd.items() if k != missing_key})
        with pytest.raises(AssertionError, match=missing_key.replace(".", r"\.")):
            ex.verify_loaded_weights()
    for key, t in (("experts.1.w2.weight_scale", torch.full((H, I // 32 + 1), 127, dtype=torch.uint8)),
                   ("experts.1.w2.weight", sd["experts.1.w1.weight"]),                       # [I, H/2] for [H, I/2]
                   ("experts.3.w1.weight", torch.zeros(I, H, dtype=torch.uint8)),            # one code a byte
                   ("experts.3.w1.weight_scale", torch.full((I,), 127, dtype=torch.uint8))):  # one scale a row
        wrong = dict(sd)
        wrong[key] = t
        ex = new()
        ex.load_state_dict(wrong)
        with pytest.raises(SlmError):
            ex.repack()
    with pytest.raises(SlmError):
        moe.MoEMxfp4Experts(H, I, E, torch.float32, "cpu")


def test_mxfp4_experts_expert_offset_selects_the_shard():
    from scalellm_amd import moe
    sd = mx.mxfp4_state_dict(H, I, E, "f16")
    ex = moe.MoEMxfp4Experts(H, I, 2, torch.float16, "cpu", expert_offset=2)
    ex.load_state_dict(sd)
    ex.repack()
    assert tuple(ex.gate_up.shape) == (2, 2 * I, H // 2) and ex.expert_offset == 2
    for e in range(2):
        assert torch.equal(ex.gate_up[e, :I], sd[f"experts.{2 + e}.w1.weight"])
        assert torch.equal(ex.gate_up_scale[e, I:], sd[f"experts.{2 + e}.w3.weight_scale"])
        assert torch.equal(ex.down[e], sd[f"experts.{2 + e}.w2.weight"])
        assert torch.equal(ex.down_scale[e], sd[f"experts.{2 + e}.w2.weight_scale"])


def test_quant_args_select_the_mxfp4_experts_class():
    from scalellm_amd import moe
    from scalellm_amd.kernels import SlmError
    from scalellm_amd.layers import QuantArgs
    q4 = QuantArgs("mxfp4", 4)
    layer = moe.FusedMoE(H, I, E, 2, q4, dtype=torch.float16, device="cpu")
    assert isinstance(layer.experts, moe.MoEMxfp4Experts)
    layer.load_state_dict(mx.mxfp4_state_dict(H, I, E, "f16"))
    layer.experts.verify_loaded_weights()
    assert tuple(layer.gate_weight.shape) == (E, H) and layer.gate_weight.dtype == torch.float16   # the router stays in T
    pg = types.SimpleNamespace(world_size=2, rank=1)
    ep = moe.ExpertParallelMoE(H, I, E, 2, pg, q4, device="cpu")
    assert isinstance(ep.experts, moe.MoEMxfp4Experts)
    assert (ep.experts.n_experts, ep.experts.expert_offset) == (2, 2)
    # the other QuantArgs fields mean nothing to mxfp4
    assert isinstance(moe.FusedMoE(H, I, E, 2, QuantArgs("mxfp4", 4, group_size=-1, desc_act=True), device="cpu").experts,
                      moe.MoEMxfp4Experts)
    for bits in (8, 16, 3):
        with pytest.raises(SlmError, match="4-bit"):
            moe.FusedMoE(H, I, E, 2, QuantArgs("mxfp4", bits), device="cpu")
        with pytest.raises(SlmError, match="4-bit"):
            moe.ExpertParallelMoE(H, I, E, 2, pg, QuantArgs("mxfp4", bits), device="cpu")
    with pytest.raises(SlmError):
        moe.FusedMoE(80, I, E, 2, q4, device="cpu")                              # hidden % 32
    with pytest.raises(SlmError):
        moe.FusedMoE(H, 80, E, 2, q4, device="cpu")                              # intermediate % 32
    assert isinstance(moe.FusedMoE(96, 160, E, 2, q4, device="cpu").experts, moe.MoEMxfp4Experts)   # % 32 is enough
    # the other selections are what they were
    assert isinstance(moe.FusedMoE(H, I, E, 2, quant_args=None, device="cpu").experts, moe.MoEDenseExperts)
    assert isinstance(moe.FusedMoE(H, I, E, 2, QuantArgs("fp8", 8), device="cpu").experts, moe.MoEFp8Experts)
    assert isinstance(moe.FusedMoE(256, 384, 8, 2, QuantArgs("awq", 4, 128), device="cpu").experts,
                      moe.MoEQuantExperts)
    with pytest.raises(SlmError):
        moe.FusedMoE(H, I, E, 2, QuantArgs("fp8", 4), device="cpu")


def test_quantize_mxfp4_weight_round_trips_per_expert():
    """quantising the dequantised experts gives the same bytes back (the grid is a fixed point), expert by expert, and
    the stacked holder dequantises to what the per-expert tensors dequantise to"""
    from scalellm_amd import kernels, moe
    sd = mx.mxfp4_state_dict(H, I, E, "bf16", seed=3)
    ex = moe.MoEMxfp4Experts(H, I, E, torch.bfloat16, "cpu")
    ex.load_state_dict(sd)
    ex.repack()
    for e in range(E):
        for w, rows in (("w1", slice(0, I)), ("w3", slice(I, 2 * I)), ("w2", None)):
            p, s = sd[f"experts.{e}.{w}.weight"], sd[f"experts.{e}.{w}.weight_scale"]
            val = kernels.dequantize_mxfp4_weight(p, s, torch.float32)
            assert np.array_equal(val.double().numpy(), mx.mref.w_as64(p, s))
            p2, s2 = kernels.quantize_mxfp4_weight(val)
            # an all-zero block may come back under another scale byte; the VALUES are what must survive
            assert np.array_equal(mx.mref.w_as64(p2, s2), mx.mref.w_as64(p, s)), (e, w)
            nz = (val.view(val.size(0), -1, 32) != 0).any(dim=2)
            assert torch.equal(s2[nz], s[nz]) and bool(nz.any())
            hp, hs = (ex.down[e], ex.down_scale[e]) if rows is None else (ex.gate_up[e, rows], ex.gate_up_scale[e, rows])
            assert torch.equal(kernels.dequantize_mxfp4_weight(hp, hs, torch.bfloat16), val.to(torch.bfloat16))
            assert torch.equal(val.to(torch.bfloat16).float(), val)            # exact in bf16


def test_model_steps_accept_the_method_and_refuse_others():
    """the constructors check quant_method before they touch the device"""
    from scalellm_amd.mixtral import MixtralDecodeStep, MixtralShape
    from scalellm_amd.qwen3 import Qwen3DecodeStep, Qwen3Shape
    for cls, shape in ((MixtralDecodeStep, MixtralShape.tiny()), (Qwen3DecodeStep, Qwen3Shape.tiny_moe())):
        with pytest.raises(ValueError, match="mxfp4"):
            cls(shape, 8, 16, 16, quant_method="mxfp8", device="cpu")
