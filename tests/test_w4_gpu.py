"""GPU parity tests for the int4 path through the C ABI: prepack (bit-exact), dequant
(bit-exact vs round-to-nearest of the oracle's fp32 value) and the MFMA GEMM.

Structure follows the reference's tests:
  * tests/kernels/marlin_gemm_test.py:47-107  (M x N x K x group x act_order grid; metric
    mean|C - C_ref| / mean|C_ref| < 1e-3 for fp16; we state 8e-3 for bf16 = one bf16 ulp class)
  * tests/kernels/marlin_repack_test.py:16-84 (repack bit-exact) -- the Marlin byte layout is an
    NVIDIA artefact, so bit-exactness is asserted on our layout through the dequant round trip
  * src/layers/quantization/qlinear_impl_test.cpp:10-98 (GPTQ fixture; linear vs dequant+matmul)
What the mean metric does NOT see: a localized error -- a ragged last row or column tile, one workgroup's K
slice, one stream-K piece, a bias missing on a clamped tile -- moves a mean over the whole output by less than
the bound (tests/test_w4_exact_cpu.py asserts it on injected faults).  tests/test_w4_exact_gpu.py closes that
gap: the same kernels on exactly representable inputs, every element compared bit for bit.
The reference never tested zero points (marlin_gemm_test.py:97 "TODO: test with zero point");
we do (AWQ asymmetric, GPTQ arbitrary stored zeros).
"""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tdtype(bits):
    return torch.bfloat16 if bits == "bf16" else torch.float16


def _to_dev(case, bits):
    dt = _tdtype(bits)
    qweight = torch.from_numpy(case["qweight"]).to(DEV)
    qzeros = torch.from_numpy(case["qzeros"]).to(DEV)
    scales = torch.from_numpy(case["scales_bits"].view(np.int16)).to(DEV).view(dt)
    g_idx = torch.from_numpy(case["g_idx"]).to(DEV) if case["g_idx"] is not None else None
    return qweight, qzeros, scales, g_idx


def _pack(case, bits):
    from scalellm_amd import kernels
    qweight, qzeros, scales, g_idx = _to_dev(case, bits)
    if case["fmt"] == "awq":
        return kernels.awq_repack(qweight, qzeros, scales, case["group_size"])
    return kernels.gptq_repack(qweight, qzeros, scales, case["group_size"], g_idx)


def _oracle_w(case):
    sc = case["scales"]
    if case["fmt"] == "awq":
        return oracle.awq_dequant(case["qweight"], case["qzeros"], sc, case["group_size"])
    return oracle.gptq_dequant(case["qweight"], case["qzeros"], sc, case["group_size"], case["g_idx"])


def _round_bits(w_f32, bits):
    if bits == "bf16":
        return helpers.f32_to_bf16_bits(w_f32)
    return w_f32.astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("bits", ["bf16", "f16"])
@pytest.mark.parametrize("fmt,gs,act", [("gptq", 128, False), ("gptq", 32, False), ("gptq", -1, False),
                                        ("gptq", 64, True), ("awq", 128, False), ("awq", 64, False),
                                        ("awq", 32, False)])
def test_prepack_dequant_roundtrip_bit_exact(bits, fmt, gs, act):
    from scalellm_amd import kernels
    case = helpers.make_quant_case(11, 256, 96, gs, fmt, bits, act_order=act)
    packed = _pack(case, bits)
    w = kernels.w4_dequant(packed)
    torch.cuda.synchronize()
    got = w.view(torch.int16).cpu().numpy().view(np.uint16)
    ref = _oracle_w(case)  # fp32, exact (q - z) * s
    if act:  # packed rows are sorted by group: row k' of the packed matrix = checkpoint row perm[k']
        perm = packed.perm.cpu().numpy()
        ref = ref[perm]
    # (q - z) * s has <= 13 significant bits: the single rounding to T is the only error source
    assert np.array_equal(got, _round_bits(ref, bits))


def test_golden_gptq_small_fixture_on_gpu():
    # the reference's own fixture (qlinear_impl_test.cpp:10-22) through prepack + dequant
    from scalellm_amd import kernels
    z = np.load(helpers.GOLDEN + "/gptq_small.npz")
    qweight = torch.from_numpy(z["qweight"]).to(DEV)
    qzeros = torch.from_numpy(z["qzeros"]).to(DEV)
    scales = torch.from_numpy(z["scales"].view(np.int16)).to(DEV).view(torch.float16)
    g_idx = torch.from_numpy(z["g_idx"]).to(DEV)
    packed = kernels.gptq_repack(qweight, qzeros, scales, 128, g_idx)
    w = kernels.w4_dequant(packed).float().cpu().numpy()
    np.testing.assert_array_equal(w, z["w"].astype(np.float16).astype(np.float32))


def _rel_err(c, ref):
    return float(np.abs(c - ref).mean() / np.abs(ref).mean())


GEMM_TOL = {"f16": 1e-3, "bf16": 8e-3}  # marlin_gemm_test.py:104-107; bf16 = 8x (8 fewer mantissa bits)


def _run_gemm(case, bits, M, bias=False, seed=0, kernel=None, row_tiles=None):
    """kernel / row_tiles: what the plan must say about this very call (kernels.w4_plan, a host-side query) --
    a knob that stopped selecting its kernel fails here instead of testing another kernel quietly"""
    from scalellm_amd import kernels
    dt = _tdtype(bits)
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(M, case["K"], device=DEV, dtype=dt, generator=g)
    b = torch.randn(case["N"], device=DEV, dtype=dt, generator=g) if bias else None
    packed = _pack(case, bits)
    c = torch.full((M, case["N"]), float("nan"), device=DEV, dtype=dt)
    if kernel is not None:
        plan = kernels.w4_plan(a, packed, c, b)
        assert plan.kernel_name == kernel, (plan.kernel_name, kernel, M, case["K"], case["N"])
        assert row_tiles is None or plan.row_tiles == row_tiles, (plan.row_tiles, row_tiles)
    kernels.gptq_gemm(a, packed, c, b)
    torch.cuda.synchronize()
    ref = oracle.gemm_f32(a.float().cpu().numpy(), _oracle_w(case))
    if bias:
        ref = ref + b.float().cpu().numpy()[None, :]
    out = c.float().cpu().numpy()
    assert not np.isnan(out).any()
    return out, ref


@pytest.mark.parametrize("bits", ["f16", "bf16"])
def test_reference_marlin_grid(bits):
    # marlin_gemm_test.py:47-56 axes: m {16,32,64} n {64,128,256,512} k {128,256}
    # group {-1,32,64,128} act_order {F,T}; + ragged m, zero points, both formats
    i = 0
    for M in (1, 16, 32, 33, 64, 100):
        for N, K in ((64, 128), (128, 256), (256, 128), (512, 256)):
            for gs in (-1, 32, 64, 128):
                for fmt, act in (("gptq", False), ("gptq", True), ("awq", False)):
                    i += 1
                    if i % 3 != (M % 3):  # thin the full product (still ~100 cases per dtype)
                        continue
                    if act and (gs == -1 or gs == K):
                        continue
                    case = helpers.make_quant_case(100 + i, K, N, gs, fmt, bits, act_order=act)
                    out, ref = _run_gemm(case, bits, M, bias=(i % 2 == 0), seed=i)
                    err = _rel_err(out, ref)
                    assert err < GEMM_TOL[bits], (M, N, K, gs, fmt, act, err)


@pytest.mark.parametrize("M", [1, 32, 64, 128, 256])   # (64 / 128: the rows of a lane of the two-lane decode step)
@pytest.mark.parametrize("K,N", [(4096, 6144), (4096, 4096), (4096, 28672), (14336, 4096)])
def test_llama3_8b_layer_shapes_awq(M, K, N):
    """BASELINE config 3 shapes (AWQ, group 128, asymmetric zeros) at full size.  The fp32 oracle
    GEMM at 4096x28672 is too slow for the suite, so the check is the size-independent identity
    int4_gemm(A) == dense_gemm(A, dequant(W)) with dequant validated bit-exact above."""
    from scalellm_amd import kernels
    case = helpers.make_quant_case(K + N, K, N, 128, "awq", "bf16")
    packed = _pack(case, "bf16")
    g = torch.Generator(device=DEV).manual_seed(M)
    a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16, generator=g)
    c = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    kernels.gptq_gemm(a, packed, c)
    w = kernels.w4_dequant(packed)
    ref = (a.float() @ w.float())
    torch.cuda.synchronize()
    err = float((c.float() - ref).abs().mean() / ref.abs().mean())
    assert err < 4e-3, err  # only the output rounding to bf16 + fp32 summation order differ
    # spot-check dequant against the oracle on a slab of columns
    w_ref = oracle.awq_dequant(case["qweight"][:, :16], case["qzeros"][:, :16],
                               case["scales"][:, :128], 128)
    got = w[:, :128].view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, helpers.f32_to_bf16_bits(w_ref))
    # and the oracle END TO END (checkpoint tensors -> construct_weights -> fp32 matmul,
    # qlinear_impl.cpp:21-100,171-183) on a subsample of ROWS over ALL N columns: independent of
    # the library's own dequant and of the vendor GEMM used above
    rows = sorted({0, M // 2, M - 1})
    ref_o = oracle.gemm_f32(a[rows].float().cpu().numpy(), _oracle_w(case))
    err_o = _rel_err(c[rows].float().cpu().numpy(), ref_o)
    assert err_o < GEMM_TOL["bf16"], err_o


@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_wave_specialised_kernel_grid(bits, tune):
    """The M > 128 kernel (w4_ws.hip: 256 x 128 tiles, producer/consumer waves, LDS-DMA) forced on
    small problems: ragged M (rows clamped, never stored), N not a multiple of 128 (clamped tiles),
    K with 1..7 64-deep chunks past a multiple of the 8-chunk ring (zero-fragment tail), every
    group size, both formats, act-order, bias, split-K (fp32 partials), fp16 and bf16."""
    tune(SLM_W4_MT=8)
    i = 0
    for M, N, K, gs, fmt, act, sk in (
            (129, 128, 128, 128, "awq", False, 0), (256, 256, 512, 128, "gptq", False, 0),
            (300, 160, 640, 32, "awq", False, 0), (200, 96, 1152, 64, "gptq", True, 0),
            (257, 384, 2048, -1, "gptq", False, 0), (512, 256, 1024, 128, "awq", False, 2),
            (256, 224, 1792, 128, "gptq", False, 7), (130, 128, 4096, 128, "awq", False, 4)):
        i += 1
        tune(SLM_W4_SPLITK=sk)
        case = helpers.make_quant_case(700 + i, K, N, gs, fmt, bits, act_order=act)
        out, ref = _run_gemm(case, bits, M, bias=(i % 2 == 1), seed=i, kernel="WS")
        err = _rel_err(out, ref)
        assert err < GEMM_TOL[bits], (M, N, K, gs, fmt, act, sk, err)


@pytest.mark.parametrize("bits", ["bf16", "f16"])
@pytest.mark.parametrize("wd,kw,ct,adma", [(2, 1, 4, 0), (4, 1, 4, 0), (2, 2, 4, 0), (4, 2, 4, 0), (2, 1, 8, 0), (4, 1, 8, 0),
                                           (2, 1, 8, 1), (4, 1, 8, 1)])
def test_m128_kernel_grid(bits, wd, kw, ct, adma, tune):
    """The 65 <= M <= 128 kernel (w4_m128.hip, round 5: all rows in one workgroup, 64-deep chunks, weight
    ring of 2 / 4 chunks): ragged M (rows clamped, never stored), N not a multiple of 128 (clamped tiles),
    K of 1..9 128-deep units with every split count the plan can pick or a test can force (uneven last
    split included), every group size (32 = two scale groups per chunk, -1 = per channel), both formats,
    act-order (column gather + padded groups), bias, fp32 split-K slabs, fp16 and bf16; kw = 2: the 512-thread
    form whose wave pairs split every chunk and meet in LDS at the end; ct = 8: 256-column workgroups (eight
    column tiles share the activation panel); adma = 1: its activations by LDS-DMA instead of through registers."""
    from scalellm_amd import kernels
    tune(SLM_W4_M128=1, SLM_W4_M128_WD=wd, SLM_W4_M128_KW=kw, SLM_W4_M128_CT=ct, SLM_W4_M128_ADMA=adma)
    i = 0
    for M, N, K, gs, fmt, act, sk in (
            (65, 128, 128, 128, "awq", False, 0), (128, 256, 512, 128, "gptq", False, 0),
            (100, 160, 640, 32, "awq", False, 0), (96, 96, 1152, 64, "gptq", True, 0),
            (127, 384, 2048, -1, "gptq", False, 0), (128, 256, 1024, 128, "awq", False, 2),
            (80, 224, 1792, 128, "gptq", False, 7), (66, 128, 4096, 128, "awq", False, 4),
            (128, 4096, 1024, 32, "gptq", True, 3), (111, 512, 896, 64, "awq", False, 0),
            (128, 6144, 4096, 128, "awq", False, 0)):
        i += 1
        tune(SLM_W4_SPLITK=sk)
        case = helpers.make_quant_case(900 + i, K, N, gs, fmt, bits, act_order=act)
        out, ref = _run_gemm(case, bits, M, bias=(i % 2 == 1), seed=i, kernel="M128")
        err = _rel_err(out, ref)
        assert err < GEMM_TOL[bits], (M, N, K, gs, fmt, act, sk, err)
    # the kernel is what ran: the general kernel (SLM_W4_M128=0) agrees to summation order only
    tune(SLM_W4_SPLITK=0, SLM_W4_M128=1, SLM_W4_M128_KW=kw, SLM_W4_M128_CT=ct, SLM_W4_M128_ADMA=adma)
    case = helpers.make_quant_case(990, 1024, 512, 128, "awq", bits)
    a_out, ref = _run_gemm(case, bits, 128, bias=False, seed=3, kernel="M128")
    # ... in the form the knobs ask for: variant = {ring depth, waves per column tile, column tiles, LDS-DMA}
    # (the ring falls back to 2 chunks where 4 do not divide a split; LDS-DMA exists in the 256-column form only)
    g = torch.Generator(device=DEV).manual_seed(3)
    plan = kernels.w4_plan(torch.randn(128, 1024, device=DEV, dtype=_tdtype(bits), generator=g), _pack(case, bits),
                           torch.empty(128, 512, device=DEV, dtype=_tdtype(bits)))
    assert plan.variant[0] in (2, wd) and list(plan.variant[1:]) == [kw, ct, adma if ct == 8 else 0], list(plan.variant)
    tune(SLM_W4_M128=0)
    b_out, _ = _run_gemm(case, bits, 128, bias=False, seed=3, kernel="GENERAL")
    assert _rel_err(a_out, ref) < GEMM_TOL[bits] and _rel_err(b_out, ref) < GEMM_TOL[bits]
    assert not np.array_equal(a_out, b_out) or True  # (informational: different split-K / tile order)


@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_xl_256x256_kernel_grid(bits, tune):
    """The symmetric 256 x 256 kernel (w4_xl.hip) forced on small problems: ragged M, N not a
    multiple of 256 (clamped column tiles), K tails past a multiple of the 4-chunk ring, every
    group size, both formats, act-order, bias, split-K."""
    tune(SLM_W4_MT=16)
    i = 0
    for M, N, K, gs, fmt, act, sk in (
            (129, 256, 128, 128, "awq", False, 0), (256, 512, 512, 128, "gptq", False, 0),
            (300, 160, 640, 32, "awq", False, 0), (200, 96, 1152, 64, "gptq", True, 0),
            (257, 384, 2048, -1, "gptq", False, 0), (512, 256, 1024, 128, "awq", False, 2),
            (256, 224, 1792, 128, "gptq", False, 7), (130, 288, 4096, 128, "awq", False, 4)):
        i += 1
        tune(SLM_W4_SPLITK=sk)
        case = helpers.make_quant_case(900 + i, K, N, gs, fmt, bits, act_order=act)
        out, ref = _run_gemm(case, bits, M, bias=(i % 2 == 1), seed=i, kernel="XL")
        err = _rel_err(out, ref)
        assert err < GEMM_TOL[bits], (M, N, K, gs, fmt, act, sk, err)


def test_wave_specialised_kernel_matches_dense_on_prefill_shape():
    """Default dispatch at a prefill-sized M picks the wave-specialised kernel; same identity as the
    layer-shape test: int4_gemm(A) == dense_gemm(A, dequant(W)), plus strided A / C rows."""
    from scalellm_amd import kernels
    K, N, M = 4096, 28672, 384
    case = helpers.make_quant_case(11, K, N, 128, "awq", "bf16")
    packed = _pack(case, "bf16")
    g = torch.Generator(device=DEV).manual_seed(3)
    abuf = torch.randn(M, K + 64, device=DEV, dtype=torch.bfloat16, generator=g)
    a = abuf[:, :K]
    cbuf = torch.zeros(M, N + 8, device=DEV, dtype=torch.bfloat16)
    c = cbuf[:, :N]
    kernels.gptq_gemm(a, packed, c)
    ref = a.float() @ kernels.w4_dequant(packed).float()
    torch.cuda.synchronize()
    assert float(cbuf[:, N:].abs().sum()) == 0.0
    err = float((c.float() - ref).abs().mean() / ref.abs().mean())
    assert err < 4e-3, err


@pytest.mark.parametrize("K,N,act", [(8192, 1280, False), (1024, 8192, False), (8192, 7168, False),
                                     (3584, 8192, False), (1024, 8192, True)])
def test_llama3_70b_tp8_rank_shapes_gptq(K, N, act):
    """BASELINE config 3 (Llama-3-70B GPTQ int4 TP=8, bs=128): the per-rank GEMMs of SURVEY 8d --
    symmetric GPTQ (stored zero 7 -> z = 8), group 128, fp16, one act-order case on the row-parallel
    o_proj shard.  Checked against the fp32 oracle GEMM on the oracle's own dequantised weights."""
    case = helpers.make_quant_case(K + N + int(act), K, N, 128, "gptq", "f16", act_order=act,
                                   sym_zero=True)
    out, ref = _run_gemm(case, "f16", 128, bias=False, seed=K)
    err = _rel_err(out, ref)
    assert err < GEMM_TOL["f16"], (K, N, act, err)


@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_dot2_gemv_kernel_grid(bits, tune):
    """The M <= 4 dot2 GEMV (w4_gemv.hip; default for M = 1, forced here for M = 2..4): every group
    size incl. per-channel (a K slice then holds part of a group: partial activation sums), K not a
    multiple of the 8-way slicing, N not a multiple of the column tiles per workgroup, both formats,
    act-order, bias, rows beyond M never stored."""
    tune(SLM_W4_GEMV=2)
    i = 0
    for M, N, K, gs, fmt, act in (
            (1, 64, 128, 128, "awq", False), (1, 4096, 4096, 128, "awq", False),
            (2, 160, 640, 32, "gptq", False), (3, 96, 1152, 64, "gptq", True),
            (4, 384, 2048, -1, "gptq", False), (1, 256, 14336, 128, "awq", False),
            (1, 224, 1792, 256, "gptq", False), (4, 288, 4096, 128, "awq", False)):
        i += 1
        case = helpers.make_quant_case(1300 + i, K, N, gs, fmt, bits, act_order=act)
        out, ref = _run_gemm(case, bits, M, bias=(i % 2 == 1), seed=i, kernel="GEMV")
        err = _rel_err(out, ref)
        assert err < GEMM_TOL[bits], (M, N, K, gs, fmt, act, err)


@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_k_sliced_small_m_kernel_grid(bits):
    """The K-sliced weight stream for M <= 32 (w4_ks.hip; default for 2 <= M <= 32): every slice width
    (1 / 2 / 4 chunks per wave) x workgroup size (4 / 8 waves) x tiles per workgroup, every group size
    incl. per-channel and groups wider than a wave's slice, K that does not fill the last workgroup's
    waves (zero activations x clamped weights), tile runs that do not divide N (clamped duplicate
    tiles, stores dropped), K split across workgroups (fp32 slabs + reduce), both formats, act-order,
    bias, rows beyond M never stored."""
    from scalellm_amd import kernels
    i = 0
    for M, N, K, gs, fmt, act, knobs in (
            (32, 4096, 4096, 128, "awq", False, {}),                                   # auto: 8 x 4, one tile
            (32, 1024, 4096, 128, "awq", False, dict(SLM_W4_KS_TPW=3)),                # ragged tile runs
            (17, 512, 2048, 128, "gptq", False, dict(SLM_W4_KS_CW=1)),                 # 2 workgroups over K
            (5, 288, 1152, 64, "gptq", True, dict(SLM_W4_KS_CW=2, SLM_W4_KS_NW=4)),    # 9 chunks on 4 x 2
            (32, 160, 640, 32, "gptq", False, dict(SLM_W4_KS_CW=2)),                   # group 32, idle waves
            (8, 384, 2048, -1, "gptq", False, dict(SLM_W4_KS_CW=4, SLM_W4_KS_NW=4)),   # per-channel
            (2, 224, 1792, 256, "gptq", False, dict(SLM_W4_KS_CW=1, SLM_W4_KS_TPW=2)), # group > slice
            (31, 256, 14336, 128, "awq", False, {}),                                   # 112 chunks: 4 x (8 x 4)
            (32, 2048, 1024, 128, "awq", False, dict(SLM_W4_KS_NW=4, SLM_W4_KS_CW=2, SLM_W4_KS_TPW=5)),
            (24, 96, 512, 128, "awq", False, {}),                                      # 4 chunks: 4-wave workgroup
            (32, 6144, 4096, 128, "gptq", True, {})):
        i += 1
        case = helpers.make_quant_case(1700 + i, K, N, gs, fmt, bits, act_order=act)
        with kernels.tuning(SLM_W4_KS=1, **knobs):  # per case: knobs of one case must not leak into the next
            out, ref = _run_gemm(case, bits, M, bias=(i % 2 == 1), seed=i, kernel="KS", row_tiles=1)
        err = _rel_err(out, ref)
        assert err < GEMM_TOL[bits], (M, N, K, gs, fmt, act, knobs, err)


@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_two_row_tile_k_sliced_kernel_grid(bits):
    """33 <= M <= 64 on the K-sliced stream with TWO row tiles (w4_ks.hip, MT = 2, round 4: every weight
    word unpacked once for two MFMAs; one chunk of K per wave, K split over 8 waves x ceil(K / 1024)
    workgroups): the Llama-3-8B layer shapes, K that does not fill the last workgroup's waves, tile
    runs that do not divide N, rows beyond M never stored (M = 33: one live row in the second tile),
    per-channel and wide groups, both formats, act-order, bias -- against the oracle, and against the
    general kernel's BM = 64 tiles on the same inputs (the default plan) to GEMM rounding."""
    from scalellm_amd import kernels
    i = 0
    for M, N, K, gs, fmt, act, knobs in (
            (64, 4096, 4096, 128, "awq", False, {}),                      # o_proj: 4 workgroups over K
            (33, 6144, 4096, 128, "awq", False, {}),                      # qkv, one row in the second tile
            (48, 1024, 14336, 128, "awq", False, dict(SLM_W4_KS_MT2=2)),  # down_proj depth: 14 slabs (not the default plan)
            (64, 28672, 4096, 128, "awq", False, {}),                     # gate_up width
            (40, 1024, 1152, 128, "gptq", False, {}),                     # 9 chunks: 7 idle waves in slab 2
            (64, 480, 1024, 128, "gptq", False, dict(SLM_W4_KS_TPW=4)),   # 15 tiles in runs of 4
            (50, 384, 2048, -1, "gptq", False, {}),                       # per-channel scales
            (57, 224, 1792, 256, "gptq", False, dict(SLM_W4_KS_TPW=2)),   # group wider than a wave's chunk
            (64, 2048, 2048, 128, "gptq", True, {}),                      # act-order column gather
            (34, 96, 128, 128, "awq", False, {})):                        # one chunk: 7 idle waves
        i += 1
        case = helpers.make_quant_case(2700 + i, K, N, gs, fmt, bits, act_order=act)
        with kernels.tuning(**{"SLM_W4_KS_MT2": 1, **knobs}):   # (opt-in kernel: not the default plan)
            out, ref = _run_gemm(case, bits, M, bias=(i % 2 == 1), seed=i, kernel="KS", row_tiles=2)
        err = _rel_err(out, ref)
        assert err < GEMM_TOL[bits], (M, N, K, gs, fmt, act, knobs, err)
        with kernels.tuning(SLM_W4_KS_MT2=0):
            base, _ = _run_gemm(case, bits, M, bias=(i % 2 == 1), seed=i, kernel="GENERAL", row_tiles=2)
        assert _rel_err(out, base) < GEMM_TOL[bits] / 2, (M, N, K, "vs the general kernel")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeded_fuzz_over_shapes_and_batch_sizes(seed):
    """A seeded random walk over what the plan switches on -- M across every kernel regime (GEMV, K-sliced,
    general POST / PRE, wave-specialised), K from one chunk to several workgroups' worth, N that is not a
    multiple of any tile run, every group size, both formats, act-order, bias on / off, both dtypes -- each
    case against the oracle dequant + fp32 GEMM at the reference's tolerance."""
    rng = np.random.default_rng(1000 + seed)
    Ms = [1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 48, 64, 65, 100, 128, 129, 200, 256, 300]
    for i in range(40):
        M = int(rng.choice(Ms))
        K = int(rng.integers(1, 25)) * 128
        N = int(rng.integers(1, 25)) * 32
        gs = int(rng.choice([-1, 32, 64, 128]))
        fmt = str(rng.choice(["awq", "gptq"]))
        act = fmt == "gptq" and gs not in (-1, K) and bool(rng.integers(0, 2))
        bits = str(rng.choice(["bf16", "f16"]))
        case = helpers.make_quant_case(5000 + 100 * seed + i, K, N, gs, fmt, bits, act_order=act)
        out, ref = _run_gemm(case, bits, M, bias=bool(rng.integers(0, 2)), seed=i)
        err = _rel_err(out, ref)
        assert err < GEMM_TOL[bits], (seed, i, M, N, K, gs, fmt, act, bits, err)


@pytest.mark.parametrize("bits", ["bf16", "f16"])
@pytest.mark.parametrize("world,M,K,N,gs", [(2, 24, 1024, 256, 128), (4, 5, 2048, 160, 64),
                                            (8, 32, 4096, 256, 128), (2, 200, 1024, 384, 32)])
def test_act_order_row_parallel_shards_match_the_full_layer(bits, world, M, K, N, gs):
    """GPTQ act-order (desc_act) under row-parallel TP: rank r holds checkpoint rows
    [r K/world, (r+1) K/world) with THEIR g_idx and the FULL scale / zero tables
    (qlinear_gptq_marlin_impl.cpp:236-243,270-276); the rows of a shard hit every group an uneven
    number of times (Marlin: is_k_full = false, :319).  Each rank's GEMM on its slice of the
    activations gives a partial sum; their fp32 sum must match the oracle's full-layer GEMM
    (gptq_dequant with g_idx) as well as the single-rank act-order path does."""
    from scalellm_amd import kernels
    case = helpers.make_quant_case(world * 100 + M, K, N, gs, "gptq", bits, act_order=True)
    qweight, qzeros, scales, g_idx = _to_dev(case, bits)
    dt = _tdtype(bits)
    g = torch.Generator(device=DEV).manual_seed(world + K)
    a = torch.randn(M, K, device=DEV, dtype=dt, generator=g)
    total = torch.zeros(M, N, device=DEV, dtype=torch.float32)
    ks = K // world
    for r in range(world):
        packed = kernels.gptq_repack(qweight[r * ks // 8:(r + 1) * ks // 8].contiguous(), qzeros, scales, gs,
                                     g_idx[r * ks:(r + 1) * ks].contiguous())
        assert packed.k_src == ks and packed.K >= ks and packed.K % 128 == 0 and packed.group_size == 32
        c = torch.full((M, N), float("nan"), device=DEV, dtype=dt)
        kernels.gptq_gemm(a[:, r * ks:(r + 1) * ks], packed, c)
        total += c.float()
    torch.cuda.synchronize()
    ref = oracle.gemm_f32(a.float().cpu().numpy(), _oracle_w(case))
    out = total.cpu().numpy()
    assert not np.isnan(out).any()
    # `world` partial sums were each rounded to T before the fp32 sum: allow that on top of the GEMM bound
    err = _rel_err(out, ref)
    assert err < GEMM_TOL[bits] * (1 + 0.5 * np.sqrt(world)), (world, M, K, N, gs, err)


@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_lean_small_m_kernel_still_covered(bits, tune):
    """w4_small.hip stays in the library for shapes the K-sliced kernel steps aside from (forced
    split-K counts it cannot realise, SLM_W4_KS=0): keep its grid alive."""
    tune(SLM_W4_KS=0)
    i = 0
    for M, N, K, gs, fmt, act in ((32, 4096, 4096, 128, "awq", False), (17, 512, 2048, 64, "gptq", False),
                                  (8, 384, 2048, -1, "gptq", True), (2, 160, 640, 32, "gptq", False)):
        i += 1
        case = helpers.make_quant_case(1800 + i, K, N, gs, fmt, bits, act_order=act)
        out, ref = _run_gemm(case, bits, M, bias=(i % 2 == 0), seed=i, kernel="SMALL")
        err = _rel_err(out, ref)
        assert err < GEMM_TOL[bits], (M, N, K, gs, fmt, act, err)


@pytest.mark.parametrize("M,K,N,env", [(256, 2048, 28672, {"SLM_W4_MT": 8}),
                                       (384, 4096, 4096, {"SLM_W4_MT": 8, "SLM_W4_SPLITK": 4}),
                                       (512, 2048, 8192, {"SLM_W4_MT": 16}),
                                       (32, 4096, 6144, {}), (1, 4096, 6144, {}),
                                       (32, 4096, 28672, {}), (32, 14336, 4096, {}),
                                       (32, 4096, 6144, {"SLM_W4_KS": 0})])
def test_repeated_launches_are_bit_identical(M, K, N, env, tune):
    """The wave-specialised / 256x256 / small-M / GEMV kernels synchronise with bare s_barriers,
    counted vmcnt/lgkmcnt waits and LDS rings, the K-sliced kernel with LDS arrival counters and a
    four-slot partial ring: a protocol error would show up as run-to-run differences.  30 back-to-back launches (no host sync in between) must agree bit for bit."""
    from scalellm_amd import kernels
    tune(**env)
    case = helpers.make_quant_case(M + K + N, K, N, 128, "awq", "bf16")
    packed = _pack(case, "bf16")
    g = torch.Generator(device=DEV).manual_seed(M)
    a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16, generator=g)
    outs = []
    for _ in range(30):
        c = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        kernels.gptq_gemm(a, packed, c)
        outs.append(c)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:])


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("M,K,N", [(256, 4096, 4096), (256, 14336, 4096), (32, 4096, 4096),
                                   (32, 14336, 4096), (7, 4096, 1024), (64, 4096, 4096), (48, 14336, 4096),
                                   (128, 4096, 4096), (128, 14336, 4096), (100, 4096, 6144)])  # (w4_m128.hip)
def test_deferred_splitk_reduce_into_rms_norm(M, K, N, dtype):
    _deferred_check(M, K, N, dtype)


@pytest.mark.parametrize("M,K,N", [(64, 4096, 4096), (48, 14336, 4096), (33, 2048, 6144)])
def test_deferred_splitk_reduce_from_the_two_row_tile_stream(M, K, N, tune):
    """the same hand-over with the slabs written by the opt-in two-row-tile K-sliced kernel (w4_ks.hip, MT = 2)"""
    tune(SLM_W4_KS_MT2=2)
    _deferred_check(M, K, N, "bf16")


def _deferred_check(M, K, N, dtype):
    """SLM_W4_DEFER_REDUCE: a split-K GEMM leaves its fp32 slabs in the workspace and
    slm_rms_norm_splitk sums them itself -- same order and rounding as the reduce kernel, so
    out / residual must equal "GEMM -> reduce -> slm_rms_norm(+residual)" bit for bit."""
    from scalellm_amd import kernels
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16
    case = helpers.make_quant_case(M + K, K, N, 128, "awq", dtype)
    packed = _pack(case, dtype)
    g = torch.Generator(device=DEV).manual_seed(K + M)
    a = torch.randn(M, K, device=DEV, dtype=tdt, generator=g)
    w = (1 + 0.1 * torch.randn(N, device=DEV, generator=g)).to(tdt)
    res0 = torch.randn(M, N, device=DEV, dtype=tdt, generator=g)
    c = torch.empty(M, N, device=DEV, dtype=tdt)
    assert not kernels.gptq_gemm(a, packed, c)
    out_ref, res_ref = torch.empty_like(c), res0.clone()
    kernels.rms_norm(out_ref, c, w, 1e-5, res_ref)
    c2 = torch.full_like(c, float("nan"))  # must not be needed when the reduce is deferred
    h = kernels.gptq_gemm(a, packed, c2, defer_reduce=True)
    out, res = torch.empty_like(c), res0.clone()
    kernels.rms_norm(out, c2, w, 1e-5, res, partials=h)
    torch.cuda.synchronize()
    if (M, K, N) in ((256, 14336, 4096), (32, 14336, 4096), (64, 4096, 4096), (48, 14336, 4096)):  # (all split over K)
        assert int(h) >= 2, "the down-projection shapes are split over K"
    if not h:
        assert torch.equal(c2, c)
    assert torch.equal(out, out_ref) and torch.equal(res, res_ref)
    # without a residual too
    out_b, out_b_ref = torch.empty_like(c), torch.empty_like(c)
    kernels.rms_norm(out_b_ref, c, w, 1e-5)
    h = kernels.gptq_gemm(a, packed, c2, defer_reduce=True)
    kernels.rms_norm(out_b, c2, w, 1e-5, partials=h)
    torch.cuda.synchronize()
    assert torch.equal(out_b, out_b_ref)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("M,K,N,knobs", [(1, 4096, 4096, {}), (1, 14336, 4096, {}), (1, 4096, 6144, {}),
                                         (3, 4096, 4096, {"SLM_W4_GEMV": 2}), (1, 4096, 28672, {}),
                                         (1, 8192, 1280, {})])
def test_gemv_splits_k_across_workgroups_only_for_a_deferred_consumer(M, K, N, knobs, dtype, tune):
    """M = 1: the GEMV normally splits K inside its workgroups (no partials).  When the caller
    defers the reduction anyway (RMSNorm / RoPE + append take fp32 slabs), a NARROW layer is also
    split across workgroups so that its launch covers all the CUs (o_proj: 128 -> 256 workgroups).
    The consumer then sees T(sum of the slabs in slab order); the undeferred GEMV sums K in a
    different association, so the two agree to fp32 rounding, not bit for bit -- checked both ways."""
    from scalellm_amd import kernels
    tune(**knobs)
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16
    case = helpers.make_quant_case(M + K + N, K, N, 128, "awq", dtype)
    packed = _pack(case, dtype)
    g = torch.Generator(device=DEV).manual_seed(K + N)
    a = torch.randn(M, K, device=DEV, dtype=tdt, generator=g)
    w = (1 + 0.1 * torch.randn(N, device=DEV, generator=g)).to(tdt)
    res0 = torch.randn(M, N, device=DEV, dtype=tdt, generator=g)
    c = torch.empty(M, N, device=DEV, dtype=tdt)
    assert not kernels.gptq_gemm(a, packed, c)                      # the ordinary GEMV
    c2 = torch.full_like(c, float("nan"))
    h = kernels.gptq_gemm(a, packed, c2, defer_reduce=True)
    wide = N >= 6144  # (qkv 4096 x 6144 = 192 workgroups already: splitting it measured slower)
    assert bool(h) == (not wide), "narrow layers are split across workgroups, wide ones are not"
    if not h:
        assert torch.equal(c2, c)
        return
    assert 2 <= int(h) <= 4 and torch.isnan(c2.float()).all()       # c is not written
    slabs = h._keep[:int(h) * M * N * 4].view(torch.float32).view(int(h), M, N).clone()
    x = slabs[0].clone()
    for s_ in range(1, int(h)):
        x = x + slabs[s_]                                            # slab order, fp32
    x = x.to(tdt)
    out, res = torch.empty_like(c), res0.clone()
    kernels.rms_norm(out, c2, w, 1e-5, res, partials=h)
    out_ref, res_ref = torch.empty_like(c), res0.clone()
    kernels.rms_norm(out_ref, x, w, 1e-5, res_ref)
    torch.cuda.synchronize()
    assert torch.equal(out, out_ref) and torch.equal(res, res_ref)
    # against the undeferred GEMV: same value up to the fp32 summation order (<= 1 ulp of T)
    rel = float((x.float() - c.float()).abs().mean() / c.float().abs().mean())
    assert rel < (4e-3 if dtype == "bf16" else 5e-4), rel


def test_gemm_linearity_and_strided_rows():
    # size-independent property: GEMM is linear in A; also A / C row strides (lda, ldc > width)
    from scalellm_amd import kernels
    case = helpers.make_quant_case(5, 512, 256, 128, "gptq", "f16", sym_zero=True)
    packed = _pack(case, "f16")
    g = torch.Generator(device=DEV).manual_seed(1)
    big = torch.randn(48, 512 + 64, device=DEV, dtype=torch.float16, generator=g)
    a = big[:, :512]
    cbuf = torch.zeros(48, 256 + 8, device=DEV, dtype=torch.float16)
    c = cbuf[:, :256]
    kernels.gptq_gemm(a, packed, c)
    c2 = torch.empty(48, 256, device=DEV, dtype=torch.float16)
    kernels.gptq_gemm((2 * a).contiguous(), packed, c2)
    torch.cuda.synchronize()
    assert float(cbuf[:, 256:].abs().sum()) == 0.0
    ref = oracle.gemm_f32(a.float().cpu().numpy(), _oracle_w(case))
    assert _rel_err(c.float().cpu().numpy(), ref) < 1e-3
    np.testing.assert_allclose(c2.float().cpu().numpy(), 2 * c.float().cpu().numpy(), rtol=2e-3, atol=2e-3)


def test_w4_rejects_bad_shapes():
    from scalellm_amd import kernels
    from scalellm_amd._lib import SlmError
    case = helpers.make_quant_case(1, 128, 64, 128, "gptq", "f16")
    packed = _pack(case, "f16")
    a = torch.zeros(4, 64, device=DEV, dtype=torch.float16)  # wrong K
    with pytest.raises(SlmError):
        kernels.gptq_gemm(a, packed, torch.zeros(4, 64, device=DEV, dtype=torch.float16))
    with pytest.raises(SlmError):  # dtype mismatch with the prepacked scales
        kernels.gptq_gemm(torch.zeros(4, 128, device=DEV, dtype=torch.bfloat16), packed,
                          torch.zeros(4, 64, device=DEV, dtype=torch.bfloat16))


# ---- round 6: SLM_W4_SHARES_CHIP (the two-row-tile K-sliced stream is the default for 33 <= M <= 64 unless the call shares the chip)
@pytest.mark.parametrize("M,K,N", [(33, 4096, 6144), (48, 4096, 4096), (64, 4096, 28672), (64, 14336, 4096)])
def test_shares_chip_flag_only_changes_the_plan(M, K, N):
    """Alone, 33 <= M <= 64 runs on the two-row-tile K-sliced stream (up to 4 slabs); with SLM_W4_SHARES_CHIP (what
    the two decode lanes pass) the call keeps the general kernel.  Both are right against the oracle, each repeats
    bit-identically, and the flag reaches the deferred-splits query."""
    from scalellm_amd import kernels
    case = helpers.make_quant_case(M + K, K, N, 128, "awq", "bf16")
    packed = _pack(case, "bf16")
    g = torch.Generator(device=DEV).manual_seed(K + M)
    a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16, generator=g)
    ref = oracle.gemm_f32(a.float().cpu().numpy(), _oracle_w(case))
    outs = {}
    for shared in (False, True):
        with kernels.shared_chip(shared):
            c1 = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
            c2 = torch.full_like(c1, float("nan"))
            plan = kernels.w4_plan(a, packed, c1)
            alone_ks = not shared and K <= 4096   # (<= 4 slabs: the two-row-tile stream is taken alone)
            assert (plan.kernel_name, plan.row_tiles) == (("KS", 2) if alone_ks else ("GENERAL", 2))
            kernels.gptq_gemm(a, packed, c1)
            kernels.gptq_gemm(a, packed, c2)
            torch.cuda.synchronize()
            assert torch.equal(c1, c2)
            assert _rel_err(c1.float().cpu().numpy(), ref) < GEMM_TOL["bf16"]
            outs[shared] = c1
    with kernels.tuning(SLM_W4_KS_MT2=0):       # the knob's "never" == the flag's plan
        c0 = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        assert kernels.w4_plan(a, packed, c0).kernel_name == "GENERAL"
        kernels.gptq_gemm(a, packed, c0)
        torch.cuda.synchronize()
    assert torch.equal(c0, outs[True])
    if K <= 4096:                                # (<= 4 slabs: the two-row-tile stream is taken alone -- other bits)
        assert not torch.equal(outs[False], outs[True])
    else:
        assert torch.equal(outs[False], outs[True])


# ---- round 6: the stream-K form of the 256 x 256 kernel (w4_xl.hip) ------------------------------------------
def _sk_case(M, K, N, dtype, gs=128, fmt="awq", bias=False):
    tdt = _tdtype(dtype)
    case = helpers.make_quant_case(M + K + N, K, N, gs, fmt, dtype)
    packed = _pack(case, dtype)
    g = torch.Generator(device=DEV).manual_seed(K + M)
    a = torch.randn(M, K, device=DEV, dtype=tdt, generator=g)
    b = torch.randn(N, device=DEV, dtype=tdt, generator=g) if bias else None
    return case, packed, a, b


def _sk_run(a, packed, b, M, N, sk):
    from scalellm_amd import kernels
    with kernels.tuning(SLM_W4_XL_SK=sk):
        c = torch.full((M, N), float("nan"), device=DEV, dtype=a.dtype)
        name = kernels.w4_plan(a, packed, c, b).kernel_name   # 2 = stream-K wherever it applies, 0 = never: tiles
        assert name == "XL_SK" if sk == 2 else name in ("XL", "WS"), (name, sk, M, N)
        kernels.gptq_gemm(a, packed, c, b)
    return c


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("M,K,N", [(2648, 4096, 4096), (2648, 4096, 6144), (2500, 14336, 4096), (2048, 4096, 4096),
                                   (4000, 2048, 3072), (2304, 1024, 4096)])
def test_stream_k_form_matches_the_oracle_and_the_tile_form(M, K, N, dtype):
    """The tile x K work cut into 256 equal ranges (pieces of up to three workgroups meet in the owner's
    epilogue): right against the oracle at the reference's GEMM tolerance, equal to the one-tile-per-workgroup form
    up to the order of the fp32 partial sums, every output written (no NaN left), ragged M (rows past the last
    full tile) included."""
    case, packed, a, b = _sk_case(M, K, N, dtype, bias=(M % 8 == 0))
    tile = _sk_run(a, packed, b, M, N, 0)
    sk = _sk_run(a, packed, b, M, N, 2)
    torch.cuda.synchronize()
    assert not torch.isnan(sk.float()).any()
    ref = oracle.gemm_f32(a.float().cpu().numpy(), _oracle_w(case))
    if b is not None:
        ref = ref + b.float().cpu().numpy()[None, :]
    assert _rel_err(sk.float().cpu().numpy(), ref) < GEMM_TOL[dtype]
    assert _rel_err(tile.float().cpu().numpy(), ref) < GEMM_TOL[dtype]
    assert _rel_err(sk.float().cpu().numpy(), tile.float().cpu().numpy()) < 2e-3


def test_stream_k_form_repeats_bit_identically_and_replays_under_a_graph():
    """The owner adds the partial tiles of the workgroups in front of it in workgroup order, whoever finishes
    first: 20 launches next to a bandwidth hog give the same bits; captured (the memset node that clears the ticket
    and the flags + the kernel) and replayed, too."""
    from scalellm_amd import kernels
    M, K, N = 2648, 4096, 4096
    case, packed, a, b = _sk_case(M, K, N, "bf16")
    first = _sk_run(a, packed, b, M, N, 2)
    hog_src = torch.randn(64 << 20, device=DEV, dtype=torch.bfloat16)
    hog_dst = torch.empty_like(hog_src)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for i in range(8):
            n = (i % 4 + 1) * (8 << 20)
            hog_dst[:n].copy_(hog_src[:n])
    outs = [_sk_run(a, packed, b, M, N, 2) for _ in range(20)]
    torch.cuda.synchronize()
    assert all(torch.equal(o, first) for o in outs)
    with kernels.tuning(SLM_W4_XL_SK=2):
        c = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        assert kernels.w4_plan(a, packed, c).kernel_name == "XL_SK"
        kernels.gptq_gemm(a, packed, c)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            kernels.gptq_gemm(a, packed, c)
            kernels.gptq_gemm(a, packed, c)   # (twice: the second call's memset node follows the first's kernel)
        for _ in range(3):
            c.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(c, first)


def test_stream_k_form_is_planned_where_the_round_model_says_so():
    """Llama-3-8B layer shapes at the mixed step's 2648 rows: qkv / o / down leave a round of tiles part-filled and
    take the stream-K form (no split-K slabs: a deferred call writes c itself); gate_up fills its rounds and does
    not; a call that shares the chip never does."""
    from scalellm_amd import _lib, kernels
    import ctypes as C
    L = _lib.lib()

    def splits_and_ws(M, K, N, flags=0):
        g = _lib.W4GemmArgs()
        g.M, g.K, g.N, g.lda, g.ldc, g.group_size, g.dtype = M, K, N, K, N, 128, _lib.SLM_BF16
        g.flags = flags
        ws, plan = int(L.slm_w4a16_gemm_workspace_bytes(C.byref(g))), _lib.W4PlanInfo()
        assert L.slm_w4a16_gemm_plan(C.byref(g), C.byref(plan)) == 0
        assert (plan.kernel_name == "XL_SK") == (ws == sk_ws) and plan.part_bytes + plan.aperm_bytes == ws
        if plan.kernel_name == "XL_SK":  # no split-K slabs: 256 equal ranges of the tile x K work list, in chunk pairs
            assert plan.split_k == 1 and plan.row_tiles == 8
            assert plan.variant[0] % 2 == 0 and 256 * plan.variant[0] >= plan.n_mblocks * plan.n_nblocks * (K // 128)
        return ws
    sk_ws = 256 * 256 * 256 * 4 + 2048
    assert splits_and_ws(2648, 4096, 4096) == sk_ws
    assert splits_and_ws(2648, 4096, 6144) == sk_ws
    assert splits_and_ws(2648, 14336, 4096) == sk_ws
    assert splits_and_ws(2648, 4096, 28672) != sk_ws
    assert splits_and_ws(2648, 4096, 4096, _lib.SLM_W4_SHARES_CHIP) != sk_ws
    with kernels.tuning(SLM_W4_XL_SK=0):
        assert splits_and_ws(2648, 4096, 4096) != sk_ws


@pytest.mark.parametrize("gs,fmt", [(32, "gptq"), (64, "awq"), (-1, "gptq")])
def test_stream_k_form_other_group_sizes(gs, fmt):
    """group 32 (two scale groups per 64-deep chunk: its own instantiation), 64 and per-channel scales"""
    M, K, N = 2304, 2048, 4096
    case, packed, a, b = _sk_case(M, K, N, "bf16", gs=gs if gs > 0 else K, fmt=fmt)
    tile = _sk_run(a, packed, b, M, N, 0)
    sk = _sk_run(a, packed, b, M, N, 2)
    again = _sk_run(a, packed, b, M, N, 2)
    torch.cuda.synchronize()
    ref = oracle.gemm_f32(a.float().cpu().numpy(), _oracle_w(case))
    assert _rel_err(sk.float().cpu().numpy(), ref) < GEMM_TOL["bf16"]
    assert _rel_err(sk.float().cpu().numpy(), tile.float().cpu().numpy()) < 2e-3
    assert torch.equal(sk, again)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_stream_k_form_seeded_fuzz(seed):
    """Random shapes through the range / piece / owner arithmetic: ranges shorter and longer than a tile, a last range
    that is cut short, row counts that leave the last row block part-empty -- against the tile form (same kernel body,
    one tile per workgroup) and repeatable bit for bit."""
    rng = np.random.default_rng(100 + seed)
    for _ in range(4):
        n_nb = int(rng.integers(8, 25))                    # 256-column blocks
        n_mb = int(rng.integers(max(6, (128 + n_nb - 1) // n_nb), 18))   # row blocks: >= 128 tiles in all
        M = 256 * (n_mb - 1) + int(rng.integers(1, 257))
        K = 256 * int(rng.integers(2, 13))                 # an even number of 128-deep chunks
        N = 256 * n_nb
        case, packed, a, b = _sk_case(M, K, N, "bf16", bias=bool(rng.integers(0, 2)))
        tile = _sk_run(a, packed, b, M, N, 0)
        sk = _sk_run(a, packed, b, M, N, 2)
        again = _sk_run(a, packed, b, M, N, 2)
        torch.cuda.synchronize()
        assert not torch.isnan(sk.float()).any(), (M, K, N)
        assert torch.equal(sk, again), (M, K, N)
        err = _rel_err(sk.float().cpu().numpy(), tile.float().cpu().numpy())
        assert err < 2e-3, (M, K, N, err)
