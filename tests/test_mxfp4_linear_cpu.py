"""CPU tests of the MXFP4 linear boundary (include/slm_hip.h section 20): exported symbols (and no workspace query),
the ctypes mirror of the argument block, argument validation before any launch, the plan under the section-13 knobs,
quantize_mxfp4_weight / dequantize_mxfp4_weight, the unpack order, the MXFP4 layer classes' loading / sharding and
the step's 4.25-bit weight accounting."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from scalellm_amd import _lib, kernels
from scalellm_amd._lib import LinearArgs, Mxfp4LinearArgs

from . import mxfp4_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")

INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT = -1, -2, -3, -5
DEFER, SILU = _lib.SLM_LINEAR_DEFER_REDUCE, _lib.SLM_LINEAR_SILU_MUL
SYMBOLS = ["slm_mxfp4_linear", "slm_mxfp4_linear_deferred_splits", "slm_mxfp4_linear_plan"]
F4 = getattr(torch, "float4_e2m1fn_x2", None)
E8 = getattr(torch, "float8_e8m0fnu", None)


@pytest.fixture(autouse=True)
def _no_knobs():
    assert _lib.lib().slm_tuning_clear(None) == 0
    yield
    assert _lib.lib().slm_tuning_clear(None) == 0


def test_the_three_symbols_are_declared_exported_and_bound_and_there_is_no_workspace_query():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"SLM_API\s+[\w\s\*]+?\b(slm_mxfp4_linear\w*)\s*\(", src)))
    assert declared == SYMBOLS
    assert not re.search(r"size_t\s+slm_mxfp4\w*workspace_bytes", src)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r"\sT\s+(slm_mxfp4_linear\w*)", out)) == set(SYMBOLS)
    L = _lib.lib()
    for n in SYMBOLS:
        assert getattr(L, n).argtypes is not None, n
    for n in ("mxfp4_linear", "mxfp4_linear_plan", "quantize_mxfp4_weight", "dequantize_mxfp4_weight"):
        assert callable(getattr(kernels, n)), n


def test_the_argument_block_matches_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(slm_mxfp4_linear_args));',
             '  printf("dense_size %zu\\n", sizeof(slm_linear_args));']
    for fname, _ in Mxfp4LinearArgs._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(slm_mxfp4_linear_args, {fname}));')
    for fname, _ in LinearArgs._fields_:
        lines.append(f'  printf("dense_{fname} %zu\\n", offsetof(slm_linear_args, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert out["size"] == C.sizeof(Mxfp4LinearArgs)
    for fname, _ in Mxfp4LinearArgs._fields_:
        assert out[fname] == getattr(Mxfp4LinearArgs, fname).offset, fname
    # slm_linear_args, field for field, then w_scale and lds
    for fname, _ in LinearArgs._fields_:
        assert out[fname] == out["dense_" + fname], fname
    assert out["w_scale"] == out["dense_size"] and out["lds"] == out["w_scale"] + 8
    assert [f for f, _ in Mxfp4LinearArgs._fields_][-2:] == ["w_scale", "lds"]


def test_validation_precedes_any_launch():
    """host address 4096 stands for every pointer: no call may reach a kernel"""
    L = _lib.lib()
    F = lambda g: L.slm_mxfp4_linear(C.byref(g), None)  # noqa: E731
    A = ref.host_args
    assert L.slm_mxfp4_linear(None, None) == INVALID
    assert F(A(8, 4096 + 16, 4096)) == UNSUPPORTED                     # K % 32
    assert F(A(8, 4096, 4096 + 16)) == UNSUPPORTED                     # N % 32
    assert F(A(8, 4096, 4096 + 32, flags=SILU)) == UNSUPPORTED         # N % 64 with SiLU
    assert F(A(8, 4096, 4096, dtype=_lib.SLM_F32)) == UNSUPPORTED      # fp32 is no activation dtype
    assert F(A(8, 4096, 4096, lda=4088)) == INVALID                    # lda < K
    assert F(A(8, 4096, 4096, ldw=2032)) == INVALID                    # ldw < K / 2
    assert F(A(8, 4096, 4096, ldw=2048 + 8)) == ALIGNMENT              # ldw % 16 (a multiple of 8 is not enough)
    assert F(A(8, 4096, 4096, ldw=2048 + 1)) == ALIGNMENT              # an odd stride
    assert F(A(8, 4096, 4096, ldw=2048 + 16)) == WORKSPACE             # ... a padded row is fine (a split plan, below)
    assert F(A(8, 4096, 4096, w=4096 + 8)) == ALIGNMENT                # W base
    assert F(A(8, 4096, 4096, w_scale=None)) == INVALID                # the block scales are required
    assert F(A(8, 4096, 4096, lds=127)) == INVALID                     # lds < K / 32
    assert F(A(8, 4096, 4096, lds=129, w_scale=4096 + 3)) == WORKSPACE  # no alignment of the scale base or stride
    assert F(A(8, 4096, 4096, lda=4096 + 1)) == ALIGNMENT              # odd strides of A and C
    assert F(A(8, 4096, 4096, ldc=4096 + 1)) == ALIGNMENT
    assert F(A(8, 4096, 4096, ldc=4088)) == INVALID                    # ldc < N
    assert F(A(8, 4096, 4096, flags=SILU, ldc=1024)) == INVALID        # ldc < N / 2
    assert F(A(8, 4096, 4096, flags=SILU | DEFER)) == INVALID          # cannot be combined
    assert F(A(8, 4096, 4096, flags=64)) == INVALID                    # unknown flag bit
    assert F(A(8, 4096, 4096, a=None)) == INVALID
    assert F(A(8, 4096, 4096, w=None)) == INVALID
    assert F(A(8, 4096, 4096, c=None)) == INVALID
    assert F(A(-1, 4096, 4096)) == INVALID
    g = A(8, 4096, 4096)
    rc, info = ref.host_plan(g)
    assert rc == 0 and info.split_k > 1
    assert F(g) == WORKSPACE                                           # a split plan without a workspace
    g.workspace, g.workspace_bytes = 4096, info.workspace_bytes - 1
    assert F(g) == WORKSPACE                                           # ... or with too small a one
    assert F(A(0, 4096, 4096)) == 0                                    # M == 0: a no-op
    assert F(A(0, 4096, 4096, a=None, c=None)) == 0
    assert L.slm_mxfp4_linear_plan(C.byref(g), None) == INVALID
    assert ref.host_plan(A(8, 4100, 4096))[0] == UNSUPPORTED
    assert L.slm_mxfp4_linear_deferred_splits(C.byref(A(8, 4100, 4096, flags=DEFER))) == 0


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
                ks = [info.slice_k_range(j) for j in range(split)]
                assert ks[0][0] == 0 and ks[-1][1] == K and all(a[1] == b[0] for a, b in zip(ks, ks[1:]))
                assert all((k1 - k0) % 128 == 0 for k0, k1 in ks[:-1])
                assert info.workspace_bytes == (split * M * N * 4 if split > 1 else 0)
                want = split if (flags & DEFER) and not bias and split >= 2 else 0
                assert L.slm_mxfp4_linear_deferred_splits(C.byref(g)) == want
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
        for K, N in ((4096, 6144), (4096, 4096), (4096, 28672), (14336, 4096), (160, 96), (672, 160)):
            for flags in (0, DEFER, SILU):
                if flags & SILU and N % 64:
                    continue
                for bias in (False, True):
                    _, dense = dense_ref.host_plan(dense_ref.host_args(M, K, N, flags=flags, bias=bias))
                    _, mx = ref.host_plan(ref.host_args(M, K, N, flags=flags, bias=bias))
                    assert bytes(dense) == bytes(mx), (M, K, N, flags, bias)


# ---- the reference, the unpack order and the quantiser ------------------------------------------------------------
def test_the_unpack_is_low_nibble_first_and_matches_the_blocks_order():
    assert ref.E2M1.tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
    # from the format: S.EE.M, bias 1
    for code in range(16):
        s, e, m = code >> 3, (code >> 1) & 3, code & 1
        v = (m / 2.0 if e == 0 else (1 + m / 2.0) * 2.0 ** (e - 1)) * (-1.0 if s else 1.0)
        assert ref.E2M1[code] == v and np.signbit(ref.E2M1[code]) == bool(s)
    # a literal 16-byte block (32 k), as a gpt-oss `*_blocks` row holds it: HF's dequantiser writes lut[byte & 0xF] to
    # the even and lut[byte >> 4] to the odd positions
    block = [0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE, 0x0F, 0x1E, 0x2D, 0x3C, 0x4B, 0x5A, 0x69, 0x78]
    want_codes = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15,
                  15, 0, 14, 1, 13, 2, 12, 3, 11, 4, 10, 5, 9, 6, 8, 7]
    packed = torch.tensor([block], dtype=torch.uint8)
    assert ref.unpack(packed)[0].tolist() == want_codes
    hf = np.empty(32)
    hf[0::2], hf[1::2] = ref.E2M1[np.array(block) & 0xF], ref.E2M1[np.array(block) >> 4]
    scale = torch.tensor([[128]], dtype=torch.uint8)
    assert np.array_equal(ref.w_as64(packed, scale)[0], 2.0 * hf)
    # the library's dequantiser: the same values, from the flat and from the blocked form
    for form in (packed, packed.view(1, 1, 16)):
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            assert np.array_equal(kernels.dequantize_mxfp4_weight(form, scale, dt).double().numpy()[0], 2.0 * hf)
    assert torch.equal(ref.pack(ref.unpack(packed)), packed)
    e255 = kernels.dequantize_mxfp4_weight(packed, torch.tensor([[255]], dtype=torch.uint8))
    assert torch.isnan(e255).all()                                      # the MX NaN


def test_mxfp4_ref_against_a_float32_matmul():
    rng = np.random.default_rng(3)
    a64, packed, scale, b64 = ref.int_inputs(rng, 5, 96, 64, True)
    w = kernels.dequantize_mxfp4_weight(packed, scale, torch.float32)
    assert np.array_equal(w.double().numpy(), ref.w_as64(packed, scale))
    want = torch.from_numpy(a64).float() @ w.T + torch.from_numpy(b64).float()[None, :]
    got = ref.mxfp4_ref(a64, packed, scale, b64)
    assert np.array_equal(got, want.double().numpy())                   # small integers: exact either way
    lo, hi = ref.mxfp4_ref(a64, packed, scale, None, (0, 32)), ref.mxfp4_ref(a64, packed, scale, None, (32, 96))
    assert np.array_equal(lo + hi, ref.mxfp4_ref(a64, packed, scale))


def test_quantize_mxfp4_weight():
    g = torch.Generator().manual_seed(7)
    # a weight already on the grid round-trips exactly (every block holds a 4 or a 6, so the rule picks its exponent back)
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 16, size=(48, 160))
    codes[:, 0::32] = rng.choice([6, 7, 14, 15], size=(48, 5))
    scale = torch.from_numpy(rng.integers(4, 251, size=(48, 5)).astype(np.uint8))   # 6 * 2^(e - 127) is finite in fp32
    packed = ref.pack(codes)
    w64 = ref.w_as64(packed, scale)
    p2, s2 = kernels.quantize_mxfp4_weight(torch.from_numpy(w64).float())
    assert p2.dtype == torch.uint8 and p2.shape == (48, 80) and s2.dtype == torch.uint8 and s2.shape == (48, 5)
    assert torch.equal(s2, scale)
    assert np.array_equal(ref.w_as64(p2, s2), w64)                      # by value: -0 may come back as +0
    # random weights over many magnitudes
    w = torch.randn(48, 160, generator=g) * torch.logspace(-6, 3, 48)[:, None]
    w[5] = 0
    w[6, 32:64] = 0
    for dt in (torch.float32, torch.bfloat16):
        wf = w.to(dt).float()
        packed, scale = kernels.quantize_mxfp4_weight(w.to(dt))
        assert ((scale >= 1) & (scale <= 254)).all()
        assert (scale[5] == 127).all() and scale[6, 1] == 127           # the all-zero block
        assert (packed[5] == 0).all() and (packed[6, 16:32] == 0).all()
        blocks = wf.reshape(48, 5, 32).double()
        amax = blocks.abs().amax(2)
        live = amax > 0
        # the shared exponent: floor(log2(amax)) - 2
        assert torch.equal(scale[live].double() - 127, torch.floor(torch.log2(amax[live])) - 2)
        deq = torch.from_numpy(ref.w_as64(packed, scale)).reshape(48, 5, 32)
        bs = torch.exp2(scale.double() - 127)[:, :, None]
        # the maximum of every block lands on 4 or 6 (amax / 2^exponent is in [4, 8): 7 saturates to 6)
        top = deq.abs().amax(2) / bs[:, :, 0]
        assert ((top[live] == 4) | (top[live] == 6)).all()
        # at most half a grid step (the grid's largest step is 2 -> 1) times the block scale, except where it saturates
        x = blocks.abs() / bs
        step = torch.where(x < 2, 0.5, torch.where(x < 4, 1.0, 2.0))
        err = (deq - blocks).abs() / bs
        assert (err[x <= 6] <= step[x <= 6] / 2).all()
        assert (deq.abs()[x > 6] == 6 * bs.expand_as(deq)[x > 6]).all()   # saturation, never a wrap
        assert (torch.sign(deq)[deq != 0] == torch.sign(blocks)[deq != 0]).all()
    # ties go to the even code; 7 and beyond saturate
    tie = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -2.5, -5.0, 7.0, 7.9, -7.5, 6.0] + [0.0] * 18)
    packed, scale = kernels.quantize_mxfp4_weight(tie[None, :])
    assert scale.item() == 127
    got = ref.w_as64(packed, scale)[0, :14]
    assert got.tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 0.0, -2.0, -4.0, 6.0, 6.0, -6.0, 6.0]
    # the exponent clamp
    tiny, huge = torch.full((1, 32), 2.0 ** -140), torch.full((1, 32), 2.0 ** 127 * 1.5)
    assert kernels.quantize_mxfp4_weight(tiny)[1].item() == 1 and kernels.quantize_mxfp4_weight(huge)[1].item() == 252
    with pytest.raises(ValueError):
        kernels.quantize_mxfp4_weight(torch.zeros(4, 48))
    with pytest.raises(ValueError):
        kernels.dequantize_mxfp4_weight(packed, torch.zeros(1, 2, dtype=torch.uint8))


# ---- the layer classes on CPU tensors ------------------------------------------------------------------------------
def _pa(rank=0, world=1):
    from scalellm_amd.model_parallel import ParallelArgs
    return ParallelArgs(rank=rank, world_size=world)


def _q(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    return kernels.quantize_mxfp4_weight(torch.randn(n, k, generator=g))


def test_the_three_accepted_dtypes_and_shapes():
    from scalellm_amd.layers import ColumnParallelMxfp4Linear
    w, sc = _q(64, 64, 0)
    forms = [(w, sc), (w.view(64, 2, 16), sc)]
    if F4 is not None and E8 is not None:
        forms += [(w.view(F4), sc.view(E8)), (w, sc.view(E8))]
    for wf, sf in forms:
        lin = ColumnParallelMxfp4Linear(64, 64, False, False, _pa(), torch.bfloat16, "cpu")
        with pytest.raises(RuntimeError, match="not loaded"):
            lin.verify_loaded_weights()
        lin.load_state_dict({"weight": wf, "weight_scale": sf, "input_scale": torch.tensor(3.0)})
        lin.verify_loaded_weights()
        assert lin.weight.dtype == torch.uint8 and lin.weight.shape == (64, 32) and torch.equal(lin.weight, w)
        assert lin.weight_scale.dtype == torch.uint8 and torch.equal(lin.weight_scale, sc)
        assert lin.weight.is_contiguous() and lin.weight_scale.is_contiguous()
    lin = ColumnParallelMxfp4Linear(64, 64, False, False, _pa(), torch.bfloat16, "cpu")
    if F4 is not None and E8 is not None:                               # the other tensor's typed dtype: swapped keys
        with pytest.raises(TypeError, match="float4_e2m1fn_x2"):
            lin.load_state_dict({"weight": w.view(E8)})
        with pytest.raises(TypeError, match="float8_e8m0fnu"):
            lin.load_state_dict({"weight_scale": sc.view(F4)})
        assert lin.weight is None and lin.weight_scale is None
    with pytest.raises(ValueError):
        lin.load_state_dict({"weight_scale": sc[:, :1]})
    with pytest.raises(TypeError):
        lin.load_state_dict({"weight_scale": torch.ones(64, 2)})
    lin.load_state_dict({"weight": w})
    with pytest.raises(RuntimeError, match="weight_scale is not loaded"):
        lin.verify_loaded_weights()
    lin.load_state_dict({"weight_scale": sc})
    with pytest.raises(RuntimeError, match="loaded twice"):
        lin.load_state_dict({"weight_scale": sc})
    with pytest.raises(RuntimeError, match="loaded twice"):
        lin.load_state_dict({"weight": w})
    with pytest.raises(kernels.SlmError):                               # no CPU fallback
        lin.forward(torch.zeros(2, 64, dtype=torch.bfloat16))


def test_a_bf16_weight_is_an_error_not_a_silent_quantisation():
    from scalellm_amd.layers import ColumnParallelMxfp4Linear, RowParallelMxfp4Linear
    w = torch.randn(64, 64).to(torch.bfloat16)
    sc = torch.full((64, 2), 127, dtype=torch.uint8)
    for cls, args in ((ColumnParallelMxfp4Linear, (64, 64, False, False)), (RowParallelMxfp4Linear, (64, 64, False, True))):
        lin = cls(*args, _pa(), torch.bfloat16, "cpu")
        with pytest.raises(TypeError, match="quantize_mxfp4_weight"):
            lin.load_state_dict({"weight": w, "weight_scale": sc})
        with pytest.raises(TypeError, match="quantize_mxfp4_weight"):
            lin.load_shard(w, sc)
        assert lin.weight is None
    fused = ColumnParallelMxfp4Linear(64, 128, False, False, _pa(), torch.bfloat16, "cpu")
    with pytest.raises(TypeError, match="quantize_mxfp4_weight"):
        fused.load_state_dict({"a.weight": w, "a.weight_scale": sc}, ["a.", "b."])


def test_the_row_parallel_k_shard_must_be_whole_blocks():
    from scalellm_amd.layers import RowParallelMxfp4Linear
    with pytest.raises(ValueError, match="32"):
        RowParallelMxfp4Linear(96, 64, False, True, _pa(0, 2), torch.bfloat16, "cpu")    # 48 per rank
    RowParallelMxfp4Linear(128, 64, False, True, _pa(0, 2), torch.bfloat16, "cpu")


def test_fused_loads_concatenate_both_tensors():
    from scalellm_amd.layers import ColumnParallelMxfp4Linear
    (qw, qs), (kw, ks), (vw, vs) = _q(64, 64, 1), _q(32, 64, 2), _q(32, 64, 3)
    prefixes = ["q_proj.", "k_proj.", "v_proj."]
    sd1 = {"v_proj.weight": vw, "v_proj.weight_scale": vs, "q_proj.bias": torch.ones(64)}
    sd2 = {"q_proj.weight": qw.view(64, 2, 16), "q_proj.weight_scale": qs, "k_proj.weight": kw,
           "k_proj.weight_scale": ks, "k_proj.bias": torch.ones(32), "v_proj.bias": torch.ones(32)}
    lin = ColumnParallelMxfp4Linear(64, 128, True, False, _pa(), torch.float16, "cpu")
    lin.load_state_dict(sd1, prefixes)
    with pytest.raises(RuntimeError, match="not loaded"):
        lin.verify_loaded_weights()
    with pytest.raises(RuntimeError, match="loaded twice"):
        lin.load_state_dict({"v_proj.weight": vw, "v_proj.weight_scale": vs}, prefixes)
    lin.load_state_dict(sd2, prefixes)
    lin.verify_loaded_weights()
    assert torch.equal(lin.weight, torch.cat([qw, kw, vw])) and torch.equal(lin.weight_scale, torch.cat([qs, ks, vs]))
    assert lin.bias.dtype == torch.float16 and lin.bias.shape == (128,)
    with pytest.raises(RuntimeError, match="loaded twice"):
        lin.load_state_dict({"q_proj.weight": qw, "q_proj.weight_scale": qs}, prefixes)
    # world 2: every prefix is cut on dim 0 before the concatenation, the scale rows with their weight rows
    (gw, gs), (uw, us) = _q(64, 64, 4), _q(64, 64, 5)
    col = ColumnParallelMxfp4Linear(64, 128, False, False, _pa(1, 2), torch.float16, "cpu", act_mul="silu")
    col.load_state_dict({"up_proj.weight": uw, "up_proj.weight_scale": us}, ["gate_proj.", "up_proj."])
    col.load_state_dict({"gate_proj.weight": gw, "gate_proj.weight_scale": gs}, ["gate_proj.", "up_proj."])
    assert col.paired and torch.equal(col.weight, torch.cat([gw[32:], uw[32:]]))
    assert torch.equal(col.weight_scale, torch.cat([gs[32:], us[32:]]))
    with pytest.raises(RuntimeError, match="without"):
        ColumnParallelMxfp4Linear(64, 128, False, False, _pa(), torch.float16, "cpu").load_state_dict(
            {"gate_proj.weight": gw}, ["gate_proj.", "up_proj."])


def test_plain_loads_shard_weight_and_scale():
    from scalellm_amd.layers import ColumnParallelMxfp4Linear, RowParallelMxfp4Linear
    w, sc = _q(128, 128, 6)
    b = torch.randn(128).to(torch.float16)
    for rank in (0, 1):
        col = ColumnParallelMxfp4Linear(128, 128, True, False, _pa(rank, 2), torch.float16, "cpu")
        col.load_state_dict({"weight": w, "weight_scale": sc, "bias": b})
        col.verify_loaded_weights()
        assert torch.equal(col.weight, w[rank * 64:(rank + 1) * 64]) and col.weight.is_contiguous()    # rows: dim 0
        assert torch.equal(col.weight_scale, sc[rank * 64:(rank + 1) * 64])                            # with their scales
        assert torch.equal(col.bias, b[rank * 64:(rank + 1) * 64])
        row = RowParallelMxfp4Linear(128, 128, True, True, _pa(rank, 2), torch.float16, "cpu")
        row.load_state_dict({"weight": w, "weight_scale": sc, "bias": b})
        row.verify_loaded_weights()
        assert torch.equal(row.weight, w[:, rank * 32:(rank + 1) * 32]) and row.weight.is_contiguous()  # k: dim 1
        assert torch.equal(row.weight_scale, sc[:, rank * 2:(rank + 1) * 2]) and row.weight_scale.is_contiguous()
        assert torch.equal(row.bias, b)                                                                 # whole
        # the shard dequantises to the columns of the whole weight
        assert torch.equal(kernels.dequantize_mxfp4_weight(row.weight, row.weight_scale),
                           kernels.dequantize_mxfp4_weight(w, sc)[:, rank * 64:(rank + 1) * 64])
        with pytest.raises(ValueError):
            row.load_state_dict({"weight": w}, ["a.", "b."])            # never fused
    lin = RowParallelMxfp4Linear(128, 128, False, True, _pa(), torch.float16, "cpu")
    lin.load_shard(w, sc)
    assert torch.equal(lin.weight_scale, sc) and lin.deferred_splits == 0 and not lin.deferred
    with pytest.raises(RuntimeError, match="loaded twice"):
        lin.load_shard(w, sc)
    with pytest.raises(ValueError):
        ColumnParallelMxfp4Linear(128, 128, False, False, _pa(), torch.float16, "cpu").load_state_dict(
            {"weight": w[:, :32].contiguous()})                         # wrong shape


def test_an_mxfp4_step_counts_four_and_a_quarter_bits_per_weight():
    from scalellm_amd.decode import LlamaShape, lane_query
    from scalellm_amd.layers import QuantArgs
    s = LlamaShape.llama3_8b()
    weights = 4096 * 6144 + 4096 * 4096 + 3 * 4096 * 14336
    q4 = lane_query(s, 32, 8, 1, -1, 128, 128, 1, 4096, weight_bits=4.25)
    assert q4.layer_weight_bytes == weights // 2 + weights // 32       # a nibble plus 1/32 scale byte
    assert lane_query(s, 32, 8, 1, -1, 128, 128, 1, 4096, weight_bits=8).layer_weight_bytes == weights
    assert "mxfp4" in QuantArgs.__doc__
