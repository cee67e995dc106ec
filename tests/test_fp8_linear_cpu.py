"""CPU tests of the fp8 linear boundary (include/slm_hip.h section 15): exported symbols, the ctypes mirror of the
argument block, argument validation before any launch, the plan under the section-13 knobs, quantize_fp8_weight, the
float64 reference itself, and the fp8 layer classes' loading / sharding."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from scalellm_amd import _lib, kernels
from scalellm_amd._lib import Fp8LinearArgs, LinearArgs

from . import fp8_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")

INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT = -1, -2, -3, -5
DEFER, SILU = _lib.SLM_LINEAR_DEFER_REDUCE, _lib.SLM_LINEAR_SILU_MUL
SYMBOLS = ["slm_fp8_linear", "slm_fp8_linear_deferred_splits", "slm_fp8_linear_plan", "slm_fp8_linear_workspace_bytes"]
F8 = torch.float8_e4m3fn


@pytest.fixture(autouse=True)
def _no_knobs():
    assert _lib.lib().slm_tuning_clear(None) == 0
    yield
    assert _lib.lib().slm_tuning_clear(None) == 0


def test_the_four_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"SLM_API\s+[\w\s\*]+?\b(slm_fp8_linear\w*)\s*\(", src)))
    assert declared == SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r"\sT\s+(slm_fp8_linear\w*)", out)) == set(SYMBOLS)
    L = _lib.lib()
    for n in SYMBOLS:
        assert getattr(L, n).argtypes is not None, n
    assert L.slm_status_string(ALIGNMENT).decode().lower().find("align") >= 0


def test_the_argument_block_matches_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(slm_fp8_linear_args));',
             '  printf("dense_size %zu\\n", sizeof(slm_linear_args));']
    for fname, _ in Fp8LinearArgs._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(slm_fp8_linear_args, {fname}));')
    for fname, _ in LinearArgs._fields_:
        lines.append(f'  printf("dense_{fname} %zu\\n", offsetof(slm_linear_args, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert out["size"] == C.sizeof(Fp8LinearArgs)
    for fname, _ in Fp8LinearArgs._fields_:
        assert out[fname] == getattr(Fp8LinearArgs, fname).offset, fname
    # slm_linear_args, field for field, then w_scale
    for fname, _ in LinearArgs._fields_:
        assert out[fname] == out["dense_" + fname], fname
    assert out["w_scale"] == out["dense_size"] and [f for f, _ in Fp8LinearArgs._fields_][-1] == "w_scale"


def test_validation_precedes_any_launch():
    """host address 4096 stands for every pointer: no call may reach a kernel"""
    L = _lib.lib()
    F = lambda g: L.slm_fp8_linear(C.byref(g), None)  # noqa: E731
    A = ref.host_args
    assert L.slm_fp8_linear(None, None) == INVALID
    assert F(A(8, 4096 + 16, 4096)) == UNSUPPORTED                     # K % 32
    assert F(A(8, 4096, 4096 + 16)) == UNSUPPORTED                     # N % 32
    assert F(A(8, 4096, 4096 + 32, flags=SILU)) == UNSUPPORTED         # N % 64 with SiLU
    assert F(A(8, 4096, 4096, dtype=_lib.SLM_F32)) == UNSUPPORTED      # fp32 is no activation dtype
    assert F(A(8, 4096, 4096, lda=4088)) == INVALID                    # lda < K
    assert F(A(8, 4096, 4096, ldw=4080)) == INVALID                    # ldw < K
    assert F(A(8, 4096, 4096, ldw=4096 + 8)) == ALIGNMENT              # ldw % 16 (a multiple of 8 is not enough)
    assert F(A(8, 4096, 4096, ldw=4096 + 16)) == WORKSPACE             # ... a padded row is fine (a split plan, below)
    assert F(A(8, 4096, 4096, w=4096 + 8)) == ALIGNMENT                # W base
    assert F(A(8, 4096, 4096, w_scale=4096 + 4)) == ALIGNMENT          # scale vector
    assert F(A(8, 4096, 4096, ldc=4088)) == INVALID                    # ldc < N
    assert F(A(8, 4096, 4096, flags=SILU, ldc=1024)) == INVALID        # ldc < N / 2
    assert F(A(8, 4096, 4096, flags=SILU | DEFER)) == INVALID          # cannot be combined
    assert F(A(8, 4096, 4096, flags=64)) == INVALID                    # unknown flag bit
    assert F(A(8, 4096, 4096, a=None)) == INVALID
    assert F(A(8, 4096, 4096, w=None)) == INVALID
    assert F(A(8, 4096, 4096, c=None)) == INVALID
    assert F(A(-1, 4096, 4096)) == INVALID
    for scale in (True, False):                                        # NULL scale = 1.0: a valid call
        g = A(8, 4096, 4096, scale=scale)
        rc, info = ref.host_plan(g)
        assert rc == 0 and info.split_k > 1
        assert F(g) == WORKSPACE                                       # a split plan without a workspace
        g.workspace, g.workspace_bytes = 4096, info.workspace_bytes - 1
        assert F(g) == WORKSPACE                                       # ... or with too small a one
    assert F(A(0, 4096, 4096)) == 0                                    # M == 0: a no-op
    assert F(A(0, 4096, 4096, a=None, c=None)) == 0
    assert L.slm_fp8_linear_plan(C.byref(g), None) == INVALID
    assert L.slm_fp8_linear_workspace_bytes(C.byref(A(8, 4100, 4096))) == 0
    assert L.slm_fp8_linear_deferred_splits(C.byref(A(8, 4100, 4096, flags=DEFER))) == 0


def test_forced_knobs_give_the_form_asked_for():
    """every row of the exact table: the plan answers (rt, nw, split); slices are whole chunks with the tail on the
    last; the workspace is split * M * N * 4; deferred_splits follows the section-13 rules"""
    L = _lib.lib()
    seen = set()
    for M, N, K, rt, nw, split, bias in ref.EXACT_CASES:
        with kernels.tuning(**ref.knobs(rt, nw, split)):
            for flags in (0, DEFER):
                g = ref.host_args(M, K, N, bias=bias, flags=flags)
                rc, info = ref.host_plan(g)
                assert rc == 0
                assert (info.row_tiles, info.waves, info.split_k) == (rt, nw, split), (M, N, K)
                assert info.n_chunks == K // 128 and info.tail_units == (K % 128) // 32
                bounds = list(info.slice_chunk[:split + 1])
                assert bounds[0] == 0 and bounds[-1] == info.n_chunks
                assert all(b1 > b0 for b0, b1 in zip(bounds, bounds[1:])) or split == 1
                ks = [info.slice_k_range(j) for j in range(split)]
                assert ks[0][0] == 0 and ks[-1][1] == K and all(a[1] == b[0] for a, b in zip(ks, ks[1:]))
                assert all((k1 - k0) % 128 == 0 for k0, k1 in ks[:-1])
                assert info.workspace_bytes == (split * M * N * 4 if split > 1 else 0)
                assert L.slm_fp8_linear_workspace_bytes(C.byref(g)) == info.workspace_bytes
                want = split if (flags & DEFER) and not bias and split >= 2 else 0
                assert L.slm_fp8_linear_deferred_splits(C.byref(g)) == want
        seen.add((rt, nw, split))
    assert seen == {(rt, nw, s) for rt, nw in ref.FORMS for s in ref.SPLITS}
    with kernels.tuning(SLM_LINEAR_SPLITK=5):                          # capped by the chunks; SiLU never splits
        assert ref.host_plan(ref.host_args(8, 256, 64))[1].split_k == 2
        assert ref.host_plan(ref.host_args(8, 4096, 128, flags=SILU))[1].split_k == 1
    with kernels.tuning(SLM_LINEAR_RT=4, SLM_LINEAR_NW=1):             # waves never fall below the row tiles
        assert ref.host_plan(ref.host_args(8, 256, 64))[1].waves == 4


def test_the_plan_is_the_dense_plan():
    from . import dense_ref
    for M in (1, 32, 64, 128, 300):
        for K, N in ((4096, 6144), (4096, 4096), (4096, 28672), (14336, 4096), (160, 96)):
            for flags in (0, DEFER, SILU):
                if flags & SILU and N % 64:
                    continue
                _, dense = dense_ref.host_plan(dense_ref.host_args(M, K, N, flags=flags))
                _, fp8 = ref.host_plan(ref.host_args(M, K, N, flags=flags))
                assert bytes(dense) == bytes(fp8), (M, K, N, flags)


# ---- the reference and the quantiser -----------------------------------------------------------------------------
def test_the_code_table_is_torchs_and_the_sweep_weight_covers_every_finite_code():
    codes = np.arange(256)
    val = ref.e4m3_value(codes)
    tv = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(F8).to(torch.float32).double().numpy()
    finite = ~np.isnan(val)
    assert finite.sum() == 254 and np.array_equal(np.isnan(tv), ~finite) and np.array_equal(val[finite], tv[finite])
    assert np.abs(val[finite]).max() == 448.0
    w = ref.code_sweep_weight().numpy()
    for n in (0, 1, 130, 255):                                         # every row, like every column, holds them all
        assert set(w[n].tolist()) | {0x7F, 0xFF} == set(range(256))
        assert set(w[:, n].tolist()) | {0x7F, 0xFF} == set(range(256))
    for bits in ref.DTYPES:                                            # every value, and half of it, is exact in T
        for s in (1.0, 0.5):
            assert np.array_equal(ref.as64(ref.rounded(val[finite] * s, bits)), val[finite] * s)


def test_fp8_ref_against_a_float32_matmul():
    g = torch.Generator().manual_seed(3)
    a = torch.randint(-4, 5, (5, 96), generator=g).float()
    w8 = (torch.randn(64, 96, generator=g) * 50).to(F8)
    scale = torch.rand(64, generator=g) + 0.5
    bias = torch.randint(-8, 9, (64,), generator=g).float()
    want = (a @ w8.to(torch.float32).T) * scale[None, :] + bias[None, :]
    got = ref.fp8_ref(a.double().numpy(), w8, scale.double().numpy(), bias.double().numpy())
    assert np.allclose(got, want.double().numpy(), rtol=1e-6, atol=1e-4)
    lo = ref.fp8_ref(a.double().numpy(), w8, None, None, (0, 32))
    hi = ref.fp8_ref(a.double().numpy(), w8, None, None, (32, 96))
    assert np.array_equal(lo + hi, ref.fp8_ref(a.double().numpy(), w8))    # small integers times e4m3: exact in float64
    assert np.array_equal(ref.w8_as64(ref.to_w8(ref.w8_as64(w8))), ref.w8_as64(w8))


def test_quantize_fp8_weight():
    g = torch.Generator().manual_seed(7)
    w = torch.randn(48, 160, generator=g) * torch.logspace(-3, 1, 48)[:, None]
    w[5] = 0
    for dt in (torch.float32, torch.bfloat16):
        w8, scale = kernels.quantize_fp8_weight(w.to(dt))
        assert w8.dtype == F8 and w8.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (48,)
        wf = w.to(dt).float()
        assert torch.equal(scale[5], torch.tensor(1.0)) and (w8[5].float() == 0).all()
        live = [i for i in range(48) if i != 5]
        assert torch.allclose(scale[live], wf[live].abs().amax(1) / 448)
        # row by row within half an e4m3 step of w / scale: 2^-4 relative for normal numbers (3 mantissa bits),
        # half the subnormal spacing 2^-9 below 2^-6
        x = (wf / scale[:, None]).double()
        err = (w8.float().double() - x).abs()
        assert (err <= torch.maximum(x.abs() * 2.0 ** -4, torch.tensor(2.0 ** -10, dtype=torch.float64)) * 1.0001).all()
        assert (w8.float().abs().amax(1)[live] == 448).all()            # the row maximum lands on the largest code
    w8, scale = kernels.quantize_fp8_weight(w, per="tensor")
    assert (scale == scale[0]).all() and torch.allclose(scale[0], w.abs().max() / 448)
    z8, zs = kernels.quantize_fp8_weight(torch.zeros(4, 32), per="tensor")
    assert (zs == 1).all() and (z8.float() == 0).all()
    with pytest.raises(ValueError):
        kernels.quantize_fp8_weight(w, per="group")


# ---- the layer classes on CPU tensors ------------------------------------------------------------------------------
def _pa(rank=0, world=1):
    from scalellm_amd.model_parallel import ParallelArgs
    return ParallelArgs(rank=rank, world_size=world)


def _q(n, k, seed, per="channel"):
    g = torch.Generator().manual_seed(seed)
    return kernels.quantize_fp8_weight(torch.randn(n, k, generator=g), per=per)


def _same(a8, b8):
    return torch.equal(a8.view(torch.uint8), b8.view(torch.uint8))


def test_scale_shapes_and_dtypes_arrive_as_fp32_per_channel():
    from scalellm_amd.layers import ColumnParallelFp8Linear
    w8, sc = _q(64, 32, 0)
    one = torch.tensor(0.375)
    for given, want in ((one, one.expand(64)), (one.reshape(1), one.expand(64)), (sc, sc), (sc[:, None], sc),
                        (sc.to(torch.bfloat16), sc.to(torch.bfloat16).float()), (one.half(), one.expand(64))):
        lin = ColumnParallelFp8Linear(32, 64, False, False, _pa(), torch.bfloat16, "cpu")
        with pytest.raises(RuntimeError, match="not loaded"):
            lin.verify_loaded_weights()
        lin.load_state_dict({"weight": w8, "weight_scale": given, "input_scale": torch.tensor(3.0)})
        lin.verify_loaded_weights()
        assert lin.weight.dtype == F8 and _same(lin.weight, w8)
        assert lin.weight_scale.dtype == torch.float32 and lin.weight_scale.is_contiguous()
        assert torch.equal(lin.weight_scale, want)
    lin = ColumnParallelFp8Linear(32, 64, False, False, _pa(), torch.bfloat16, "cpu")
    with pytest.raises(ValueError):
        lin.load_state_dict({"weight_scale": sc[:32]})
    with pytest.raises(TypeError):
        lin.load_state_dict({"weight_scale": torch.ones(64, dtype=torch.int32)})
    lin.load_state_dict({"weight": w8})
    with pytest.raises(RuntimeError, match="weight_scale is not loaded"):
        lin.verify_loaded_weights()
    lin.load_state_dict({"weight_scale": sc})
    with pytest.raises(RuntimeError, match="loaded twice"):
        lin.load_state_dict({"weight_scale": sc})
    with pytest.raises(RuntimeError, match="loaded twice"):
        lin.load_state_dict({"weight": w8})
    with pytest.raises(kernels.SlmError):                               # no CPU fallback
        lin.forward(torch.zeros(2, 32, dtype=torch.bfloat16))


def test_a_bf16_weight_is_an_error_not_a_silent_quantisation():
    from scalellm_amd.layers import ColumnParallelFp8Linear, RowParallelFp8Linear
    w = torch.randn(64, 32).to(torch.bfloat16)
    for cls, args in ((ColumnParallelFp8Linear, (32, 64, False, False)), (RowParallelFp8Linear, (32, 64, False, True))):
        lin = cls(*args, _pa(), torch.bfloat16, "cpu")
        with pytest.raises(TypeError, match="float8_e4m3fn"):
            lin.load_state_dict({"weight": w, "weight_scale": torch.ones(64)})
        with pytest.raises(TypeError, match="float8_e4m3fn"):
            lin.load_shard(w, torch.ones(64))
        assert lin.weight is None
    fused = ColumnParallelFp8Linear(32, 128, False, False, _pa(), torch.bfloat16, "cpu")
    with pytest.raises(TypeError, match="float8_e4m3fn"):
        fused.load_state_dict({"a.weight": w, "a.weight_scale": torch.ones(1)}, ["a.", "b."])


def test_fused_loads_expand_each_shards_own_scale():
    from scalellm_amd.layers import ColumnParallelFp8Linear
    (q8, qs), (k8, ks), (v8, vs) = _q(64, 32, 1, "tensor"), _q(32, 32, 2, "tensor"), _q(32, 32, 3)
    prefixes = ["q_proj.", "k_proj.", "v_proj."]
    sd1 = {"v_proj.weight": v8, "v_proj.weight_scale": vs[:, None], "q_proj.bias": torch.ones(64)}
    sd2 = {"q_proj.weight": q8, "q_proj.weight_scale": qs[0], "k_proj.weight": k8, "k_proj.weight_scale": ks[:1],
           "k_proj.bias": torch.ones(32), "v_proj.bias": torch.ones(32), "k_proj.input_scale": torch.tensor(2.0)}
    lin = ColumnParallelFp8Linear(32, 128, True, False, _pa(), torch.float16, "cpu")
    lin.load_state_dict(sd1, prefixes)
    with pytest.raises(RuntimeError, match="not loaded"):
        lin.verify_loaded_weights()
    with pytest.raises(RuntimeError, match="loaded twice"):
        lin.load_state_dict({"v_proj.weight": v8, "v_proj.weight_scale": vs}, prefixes)
    lin.load_state_dict(sd2, prefixes)
    lin.verify_loaded_weights()
    assert _same(lin.weight, torch.cat([q8.view(torch.uint8), k8.view(torch.uint8), v8.view(torch.uint8)]))
    assert torch.equal(lin.weight_scale, torch.cat([qs[:1].expand(64), ks[:1].expand(32), vs]))
    assert lin.bias.dtype == torch.float16 and lin.bias.shape == (128,)
    with pytest.raises(RuntimeError, match="loaded twice"):
        lin.load_state_dict({"q_proj.weight": q8, "q_proj.weight_scale": qs}, prefixes)
    # world 2: every prefix is cut on dim 0 before the concatenation, the scale with its rows
    (g8, gs), (u8, us) = _q(64, 32, 4), _q(64, 32, 5, "tensor")
    col = ColumnParallelFp8Linear(32, 128, False, False, _pa(1, 2), torch.float16, "cpu", act_mul="silu")
    col.load_state_dict({"up_proj.weight": u8, "up_proj.weight_scale": us[0]}, ["gate_proj.", "up_proj."])
    col.load_state_dict({"gate_proj.weight": g8, "gate_proj.weight_scale": gs}, ["gate_proj.", "up_proj."])
    assert col.paired and _same(col.weight, torch.cat([g8.view(torch.uint8)[32:], u8.view(torch.uint8)[32:]]))
    assert torch.equal(col.weight_scale, torch.cat([gs[32:], us[:32]]))
    with pytest.raises(RuntimeError, match="without"):
        ColumnParallelFp8Linear(32, 128, False, False, _pa(), torch.float16, "cpu").load_state_dict(
            {"gate_proj.weight": g8}, ["gate_proj.", "up_proj."])


def test_plain_loads_shard_weight_and_scale():
    from scalellm_amd.layers import ColumnParallelFp8Linear, RowParallelFp8Linear
    w8, sc = _q(128, 64, 6)
    b = torch.randn(128).to(torch.float16)
    for rank in (0, 1):
        col = ColumnParallelFp8Linear(64, 128, True, False, _pa(rank, 2), torch.float16, "cpu")
        col.load_state_dict({"weight": w8, "weight_scale": sc, "bias": b})
        col.verify_loaded_weights()
        assert _same(col.weight, w8[rank * 64:(rank + 1) * 64]) and col.weight.is_contiguous()     # rows: dim 0
        assert torch.equal(col.weight_scale, sc[rank * 64:(rank + 1) * 64])                        # with their scales
        assert torch.equal(col.bias, b[rank * 64:(rank + 1) * 64])
        row = RowParallelFp8Linear(64, 128, True, True, _pa(rank, 2), torch.float16, "cpu")
        row.load_state_dict({"weight": w8, "weight_scale": sc[:, None].double(), "bias": b})
        row.verify_loaded_weights()
        assert _same(row.weight, w8[:, rank * 32:(rank + 1) * 32]) and row.weight.is_contiguous()  # columns: dim 1
        assert torch.equal(row.weight_scale, sc) and torch.equal(row.bias, b)                      # whole
        with pytest.raises(ValueError):
            row.load_state_dict({"weight": w8}, ["a.", "b."])           # never fused
    lin = RowParallelFp8Linear(64, 128, False, True, _pa(), torch.float16, "cpu")
    lin.load_shard(w8, sc[0])                                           # per tensor -> expanded
    assert torch.equal(lin.weight_scale, sc[:1].expand(128)) and lin.deferred_splits == 0 and not lin.deferred
    with pytest.raises(RuntimeError, match="loaded twice"):
        lin.load_shard(w8, sc)
    with pytest.raises(ValueError):
        ColumnParallelFp8Linear(64, 128, False, False, _pa(), torch.float16, "cpu").load_state_dict(
            {"weight": w8[:, :32].contiguous()})                        # wrong shape


def test_an_fp8_step_counts_one_byte_per_weight():
    from scalellm_amd.decode import LlamaShape, lane_query
    s = LlamaShape.llama3_8b()
    q8 = lane_query(s, 32, 8, 1, -1, 128, 128, 1, 4096, weight_bits=8)
    assert q8.layer_weight_bytes == 4096 * 6144 + 4096 * 4096 + 3 * 4096 * 14336
