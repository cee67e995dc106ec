"""Bit-exact tests of the int4 GEMM family on inputs whose result is exactly representable.

The functional tests of these kernels (test_w4_gpu.py, test_w8_gpu.py, test_moe_gpu.py) bound a MEAN relative error,
which a localized fault -- a ragged last tile, one workgroup's K slice, one stream-K piece, a bias missing on a
clamped tile, a scattered MoE row -- passes (tests/test_w4_exact_cpu.py shows it).  Here the inputs are chosen so that
every product and every partial sum is representable in fp32 (tests/helpers.py: small-integer activations,
power-of-two scales, a bias that is a multiple of the smallest scale; tests/w4_exact_cases.py: the shapes, asserted
against the exactness budget).  The result then does not depend on summation order, split-K, stream-K pieces, slabs or
the dequant form, and every kernel owes RNE_T(exact sum + bias) in EVERY element, bit for bit: no tolerance, no element
left out.  The reference is a float64 matmul of integer-valued arrays.

Every case first asks the plan query which kernel, row tiles, split and variant will run and asserts the intended one.
What this proves is structure and indexing; the rounding of non-trivial scales and f16 output rounding without a bias
stay with the random-data tests.  Each test prints the share of its outputs that are not representable in T, i.e.
that exercise the epilogue's rounding, and asserts that it is above zero wherever the recipe owes it
(cases.assert_share: every bf16 truth over K >= 512, every f16 truth with the big bias).
"""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import moe_ref
from tests import w4_exact_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}


def _dev(x, bits):
    """small integers times powers of two: exact in T (asserted by the budget for the bias)"""
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(TDT[bits])


def _t_of(truth, bits):
    return torch.from_numpy(truth).to(TDT[bits]).to(DEV)


def _nan(shape, bits):
    return torch.full(shape, float("nan"), device=DEV, dtype=TDT[bits])


def _report(name, bits, shares):
    print(f"\n[exact] {name} {bits}: share of outputs needing rounding " + " ".join(f"{s:.3f}" for s in shares))


def _run_group_case(group, case, bits):
    """plan asserted, GEMM into a NaN-filled c, every element against the truth; returns the rounding share"""
    from scalellm_amd import kernels
    q, a_np, b_np, truth, share = cases.inputs(bits, case)
    a, b = _dev(a_np, bits), _dev(b_np, bits)
    packed = helpers.pack_case(q, bits)
    c = _nan((case.M, case.N), bits)
    what = f"{group.name} {bits} {tuple(case[:7])} {case.knobs}"
    with kernels.tuning(**{**group.knobs, **case.knobs}):
        cases.check_plan(group, case, kernels.w4_plan(a, packed, c, b))
        kernels.gptq_gemm(a, packed, c, b)
    torch.cuda.synchronize()
    helpers.assert_bits_equal(c, truth, TDT[bits], what)
    cases.assert_share(bits, case.K, case.bias, share, what)
    return share


DENSE = cases.dense_groups()


@pytest.mark.parametrize("bits", cases.BITS)
@pytest.mark.parametrize("group", DENSE, ids=[g.name for g in DENSE])
def test_kernel_is_exact(group, bits):
    """GEMV, the K-sliced stream with one and two row tiles, the lean small-M kernel, the general kernel over
    {row tiles, POST, PC, SPLITK}, w4_m128.hip over its eight forms, the wave-specialised and the 256 x 256 kernel:
    one case per kernel, variant tuple and dtype, looping over its shapes"""
    shares = [_run_group_case(group, case, bits) for case in cases.cases_of(group, bits)]
    assert shares
    _report(group.name, bits, shares)


def test_lean_kernel_shapes_are_the_grouped_kernels():
    from tests.test_moe_gpu import STREAM_CASES
    assert [s[1:] for s in cases.STREAM_SHAPES] == [c[2:5] for c in STREAM_CASES]


@pytest.mark.parametrize("bits", cases.BITS)
def test_gemv_deferred_slabs_sum_to_the_truth_in_fp32(bits):
    """M = 1 with a deferred reduction: a narrow layer is split across workgroups and leaves fp32 slabs
    (test_gemv_splits_k_across_workgroups_only_for_a_deferred_consumer reads them the same way).  Each slab is an
    exact partial sum, so their fp32 sum in slab order is the truth itself, before any rounding to T."""
    from scalellm_amd import kernels
    M, N, K, knobs = cases.GEMV_DEFERRED[bits]
    q, a_np, _, truth, _ = cases.inputs(bits, cases._c(M, N, K, 128, "awq"))
    a, packed = _dev(a_np, bits), helpers.pack_case(q, bits)
    c = _nan((M, N), bits)
    with kernels.tuning(**knobs):
        plan = kernels.w4_plan(a, packed, c, defer_reduce=True)
        assert plan.kernel_name == "GEMV" and 2 <= plan.split_k <= 4, (plan.kernel_name, plan.split_k)
        h = kernels.gptq_gemm(a, packed, c, defer_reduce=True)
    torch.cuda.synchronize()
    assert int(h) == plan.split_k and bool(torch.isnan(c.float()).all())    # c is not written
    slabs = h._keep[:int(h) * M * N * 4].view(torch.float32).view(int(h), M, N).clone()
    x = slabs[0].clone()
    for s in range(1, int(h)):
        x = x + slabs[s]
    bad = np.flatnonzero(x.cpu().numpy().reshape(-1) != truth.astype(np.float32).reshape(-1))
    assert bad.size == 0, (bad.size, bad[:8].tolist())
    assert bool((slabs != 0).any(dim=2).all())                               # every slab carries a part of K


@pytest.mark.parametrize("bits", cases.BITS)
@pytest.mark.parametrize("n", range(len(cases.XL_SK)))
def test_stream_k_and_tile_form_are_exact(n, bits):
    """the tile x K work list cut into 256 ranges whose pieces meet in the owner's epilogue, and the
    one-tile-per-workgroup forms on the same inputs (what SLM_W4_XL_SK=0 plans by itself, and the 256 x 256 kernel
    that the stream-K form is a variant of): all exact, hence equal to each other"""
    from scalellm_amd import kernels
    case = cases.XL_SK[n]
    q, a_np, b_np, truth, share = cases.inputs(bits, case)
    a, b, packed = _dev(a_np, bits), _dev(b_np, bits), helpers.pack_case(q, bits)
    for form, knobs, kernel in cases.XL_SK_FORMS:
        c = _nan((case.M, case.N), bits)
        with kernels.tuning(**knobs):
            plan = kernels.w4_plan(a, packed, c, b)
            cases.check_xl_plan(case, kernel, plan)
            kernels.gptq_gemm(a, packed, c, b)
        torch.cuda.synchronize()
        helpers.assert_bits_equal(c, truth, TDT[bits], f"{form} {bits} {tuple(case[:7])} as {plan.kernel_name}")
    cases.assert_share(bits, case.K, case.bias, share, case)
    _report("XL_SK-%d" % n, bits, [share])


@pytest.mark.parametrize("bits", cases.BITS)
@pytest.mark.parametrize("world,M,N,K,gs", cases.SHARDS)
def test_act_order_row_parallel_shards_are_exact(world, M, N, K, gs, bits):
    """each rank's c against its own partial truth: the rows of its shard with the full scale table"""
    from scalellm_amd import kernels
    q, a_np, _, truth, _ = cases.inputs(bits, cases._c(M, N, K, gs, "gptq", act=True))
    parts = cases.shard_truths(q, a_np, world)
    a = _dev(a_np, bits)
    qweight = torch.from_numpy(q["qweight"]).to(DEV)
    qzeros = torch.from_numpy(q["qzeros"]).to(DEV)
    scales = torch.from_numpy(q["scales_bits"].view(np.int16)).to(DEV).view(TDT[bits])
    g_idx = torch.from_numpy(q["g_idx"]).to(DEV)
    ks = K // world
    shares = []
    for r in range(world):
        helpers.assert_exact_budget(a_np[:, r * ks:(r + 1) * ks], cases.shard_case(q, r, world))
        packed = kernels.gptq_repack(qweight[r * ks // 8:(r + 1) * ks // 8].contiguous(), qzeros, scales, gs,
                                     g_idx[r * ks:(r + 1) * ks].contiguous())
        assert packed.k_src == ks and packed.K >= ks and packed.group_size == 32
        c = _nan((M, N), bits)
        a_r = a[:, r * ks:(r + 1) * ks]
        what = f"shard {r} of {world} {bits} {(M, N, K, gs)}"
        cases.check_shard_plan(packed.K, kernels.w4_plan(a_r, packed, c), what)
        kernels.gptq_gemm(a_r, packed, c)
        torch.cuda.synchronize()
        helpers.assert_bits_equal(c, parts[r], TDT[bits], what)
        shares.append(cases.share_of(parts[r], bits))
        cases.assert_share(bits, ks, False, shares[-1], what)      # the rank's own K; a partial sum has no bias
    _report("shards-%d-of-%s" % (world, (M, N, K, gs)), bits, shares)


@pytest.mark.parametrize("bits", cases.BITS)
@pytest.mark.parametrize("group", cases.STRIDED, ids=[g.name for g in cases.STRIDED])
def test_strided_views_are_exact_and_guards_untouched(group, bits):
    """A and C as column slices of wider buffers (lda > K, ldc > N); the columns beside c and the row below it keep
    their NaN, the columns beside a hold values that would wreck the sums"""
    from scalellm_amd import kernels
    case, = cases.cases_of(group, bits)
    q, a_np, b_np, truth, share = cases.inputs(bits, case)
    abuf = torch.full((case.M, case.K + 64), 3.0, device=DEV, dtype=TDT[bits])
    abuf[:, :case.K] = _dev(a_np, bits)
    a, b, packed = abuf[:, :case.K], _dev(b_np, bits), helpers.pack_case(q, bits)
    cbuf = _nan((case.M + 1, case.N + 8), bits)
    c = cbuf[:case.M, :case.N]
    with kernels.tuning(**{**group.knobs, **case.knobs}):
        cases.check_plan(group, case, kernels.w4_plan(a, packed, c, b))
        kernels.gptq_gemm(a, packed, c, b)
    torch.cuda.synchronize()
    helpers.assert_bits_equal(c, truth, TDT[bits], f"{group.name} {bits}")
    assert bool(torch.isnan(cbuf[:, case.N:]).all()) and bool(torch.isnan(cbuf[case.M]).all())
    cases.assert_share(bits, case.K, case.bias, share, group.name)
    _report(group.name, bits, [share])


# (a K = 4096 row has no f16 case)
SILU = [(g, bits) for g in cases.SILU for bits in cases.BITS if cases.cases_of(g, bits)]


@pytest.mark.parametrize("group,bits", SILU, ids=["%s-%s" % (g.name, bits) for g, bits in SILU])
def test_fused_silu_mul_is_exact(group, bits):
    """paired prepack + the SiLU * mul epilogue: gate and up are rounded exactly, so the fused output must equal
    kernels.silu_and_mul (the project's own activation, tested in test_glue_gpu.py) of T(truth) bit for bit; the plain
    GEMM under the same knobs against the truth itself"""
    from scalellm_amd import kernels
    shares = []
    for case in cases.cases_of(group, bits):
        q, a_np, b_np, truth, share = cases.inputs(bits, case)
        M, N = case.M, case.N
        a, b = _dev(a_np, bits), _dev(b_np, bits)
        plain, paired = helpers.pack_case(q, bits), helpers.pack_case(q, bits, paired=True)
        want = torch.empty(M, N // 2, device=DEV, dtype=TDT[bits])
        kernels.silu_and_mul(want, _t_of(truth, bits))
        b_packed = b[torch.from_numpy(cases.paired_src_cols(N)).to(DEV)].contiguous() if b is not None else None
        full, got = _nan((M, N), bits), _nan((M, N // 2), bits)
        what = f"{group.name} {bits} {tuple(case[:7])}"
        with kernels.tuning(**{**group.knobs, **case.knobs}):
            cases.check_plan(group, case, kernels.w4_plan(a, plain, full, b))
            cases.check_plan(group, case, kernels.w4_plan(a, paired, got, b_packed, silu_mul=True))
            kernels.gptq_gemm(a, plain, full, b)
            kernels.gptq_gemm(a, paired, got, b_packed, silu_mul=True)
        torch.cuda.synchronize()
        helpers.assert_bits_equal(full, truth, TDT[bits], what + " plain")
        helpers.assert_bits_equal(got, want.double().cpu().numpy(), TDT[bits], what + " fused")
        cases.assert_share(bits, case.K, case.bias, share, what)    # gate and up both round
        shares.append(share)
    assert shares
    _report(group.name, bits, shares)


@pytest.mark.parametrize("bits", cases.BITS)
@pytest.mark.parametrize("n", range(cases.W8_N))
def test_8bit_planes_are_exact(n, bits):
    """8-bit layers (two int4 planes over 2K rows, the high plane with 16 s) through the default plan at one M per
    kernel regime; one scale value per case, as the budget (x 32) requires"""
    from scalellm_amd import kernels
    shares, seen = [], set()
    for M in cases.W8_M:
        q, a_np, b_np, truth, share = cases.inputs8(bits, n, M)
        a, b, packed = _dev(a_np, bits), _dev(b_np, bits), helpers.pack_case8(q, bits)
        assert packed.K == 2 * q["K"]
        c = _nan((M, q["N"]), bits)
        plan = kernels.w4_plan(a, packed, c, b)
        what = f"w8 {bits} {cases.W8_CASES[bits][n]} M={M} as {plan.kernel_name}"
        cases.check_w8_plan(M, packed.K, packed.group_size, plan, what)
        seen.add(plan.kernel_name)
        kernels.gptq_gemm(a, packed, c, b)
        torch.cuda.synchronize()
        helpers.assert_bits_equal(c, truth, TDT[bits], what)
        cases.assert_share(bits, q["K"], b is not None, share, what)
        shares.append(share)
    assert seen == {"GEMV", "KS", "GENERAL"}
    _report("w8-%d" % n, bits, shares)


def _aligned(ids_np, E):
    """the aligned block list of moe_ref in buffers of the capacity size (test_moe_gpu._aligned)"""
    from scalellm_amd import kernels
    cap, blocks = kernels.moe_align_capacity(ids_np.size, E, 32)
    rs, re_, rn, _ = moe_ref.align_block(ids_np, E, 32)
    srt = np.full(cap, ids_np.size, np.int32)
    eid = np.zeros(blocks, np.int32)
    srt[:rn], eid[:rn // 32] = rs, re_
    return (torch.from_numpy(srt).to(DEV), torch.from_numpy(eid).to(DEV),
            torch.tensor([rn], dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("bits", cases.BITS)
@pytest.mark.parametrize("n", range(len(cases.MOE)))
def test_moe_grouped_gemm_is_exact(n, bits):
    """every scattered row of the grouped GEMM: the token matrix (a_div = k), one row per (token, expert) with a
    power-of-two row scale (a_div = 1), and paired experts with the SiLU * mul epilogue; the guard row below c
    untouched, no NaN left"""
    from scalellm_amd import _lib, kernels
    T_, k, K, N, gs = cases.MOE[n]
    experts, ids, a_tok, a_flat, row_scale = cases.moe_inputs(bits, n)
    code = _lib.SLM_W4_AWQ if experts[0]["fmt"] == "awq" else _lib.SLM_W4_GPTQ
    plain = kernels.moe_stack_experts([helpers.pack_case(q, bits) for q in experts], code)
    paired = kernels.moe_stack_experts([helpers.pack_case(q, bits, paired=True) for q in experts], code)
    srt, eid, npad = _aligned(ids, cases.MOE_E)
    n_flat, what = T_ * k, f"moe {bits} {cases.MOE[n]}"
    truth_k = cases.moe_truth(experts, ids, a_tok, k)
    full = _nan((n_flat + 1, N), bits)
    kernels.moe_w4_grouped_gemm(_dev(a_tok, bits), plain, full[:n_flat], srt, eid, npad, k)
    helpers.assert_bits_equal(full[:n_flat], truth_k, TDT[bits], what + " a_div=k")
    assert bool(torch.isnan(full[n_flat]).all())
    truth_1 = cases.moe_truth(experts, ids, a_flat, 1) * row_scale[:, None].astype(np.float64)
    full = _nan((n_flat + 1, N), bits)
    kernels.moe_w4_grouped_gemm(_dev(a_flat, bits), plain, full[:n_flat], srt, eid, npad, 1,
                                row_scale=torch.from_numpy(row_scale).to(DEV))
    helpers.assert_bits_equal(full[:n_flat], truth_1, TDT[bits], what + " a_div=1 row_scale")
    assert bool(torch.isnan(full[n_flat]).all())
    want = torch.empty(n_flat, N // 2, device=DEV, dtype=TDT[bits])
    kernels.silu_and_mul(want, _t_of(truth_k, bits))
    half = _nan((n_flat + 1, N // 2), bits)
    kernels.moe_w4_grouped_gemm(_dev(a_tok, bits), paired, half[:n_flat], srt, eid, npad, k, silu_mul=True)
    helpers.assert_bits_equal(half[:n_flat], want.double().cpu().numpy(), TDT[bits], what + " silu")
    assert bool(torch.isnan(half[n_flat]).all())
    shares = [cases.share_of(t, bits) for t in (truth_k, truth_1)]
    for share in shares:                        # (the experts carry no bias: nothing is owed in f16)
        cases.assert_share(bits, K, False, share, what)
    _report("moe-%d" % n, bits, shares)
