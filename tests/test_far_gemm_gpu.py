"""Linears whose A, W (with the MXFP4 block scales) or C reach past 2 GiB and 4 GiB through the row stride: one far
operand per launch, a strided view that starts at the 4 GiB mark of tests/far_arena.py's arena (the base of region K)
with far_arena.far_ld() as lda / ldw (lds) / ldc, so that the rows in between cross 2^31 and the last row lies past
2^32; the other operands are small ordinary tensors.  Dense, fp8 and mxfp4 linears at M = 33, N = 96, K = 672 with 1
and 3 K slices, integer inputs as in test_exact_on_small_integers (every partial sum exact in fp32 in any order).
Every result is bit-equal to the compact call and to the float64 integer truth, rounded once; a far C leaves
everything else in the arena poisoned.

The address arithmetic the far strides exercise (csrc/dense.hip and its weight-stream header): (int64_t)gm * p.lda and
(int64_t)gm * p.ldc for the rows of A and C, ncol * p.ldw (and ncol * p.lds) for the weight rows and the block scales.
tests/test_far_offsets_cpu.py checks the alias condition of these strides and that the three 32-bit slips would change
a row.

The int4 GEMM (w4_plan.hip: a_fits_i31 / c_fits_i31) runs with a far A at M = 33 and M = 129 and with a far C, on the
fall-back kernel that test_far_offsets_cpu.py's W4_FAR_PLANS names, against the float64 truth of w4_exact_cases.

The grouped MoE GEMMs (moe_gemm.hip: "the expert base is a 64-bit pointer, offsets inside an expert 32-bit"; dense, fp8
and mxfp4, each with its own weight stream) run three experts behind w_expert_stride -- and the fp8 column scales /
mxfp4 block scales behind w_scale_expert_stride, in region V -- in two layouts: "past" (far_ld: expert 1 past 2^31,
expert 2 past 2^32, every alias poison) and "across" (across_stride: the offsets inside expert 1 cross 2^31, inside
expert 2 cross 2^32; aliases fall into other experts, which hold other values); and far A / far C rows via lda / ldc;
with and without SiLU.mul: bit-equal to the compact call, and without SiLU to the integer truth.

The fp8 linear takes a real column-scale vector (powers of two): a contiguous [N] tensor has no stride to make far, but
the epilogue's scale read stays in the picture."""
import numpy as np
import pytest
import torch

from tests import dense_ref, helpers, mxfp4_ref
from tests import far_arena as F
from tests import glue_ref as ref
from tests import w4_exact_cases as w4
from tests.test_far_offsets_cpu import W4_FAR_PLANS

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
M, N, K = F.GEMM_M, F.GEMM_N, F.GEMM_K
KINDS = ("dense", "fp8", "mxfp4")
FAR = ("A", "W", "C")


@pytest.fixture(scope="module")
def arena():
    torch.cuda.reset_peak_memory_stats()
    holder = [F.allocate()]
    yield holder[0]
    holder.clear()
    torch.cuda.empty_cache()
    print(f"FAR-ARENA gemm: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _far_view(arena, dtype, rows, cols, base=F.K_BASE):
    """([rows, cols] view of the arena with row stride far_ld, element ranges of the arena (int16 units) it covers)"""
    flat = arena.view(dtype)
    es = flat.element_size()
    ld = F.far_ld(rows, es)
    v = torch.as_strided(flat, (rows, cols), (ld, 1), storage_offset=base // es)
    spans = [((base + r * ld * es) // 2, (base + r * ld * es + cols * es + 1) // 2) for r in range(rows)]
    return v, spans


def _put(view, small):
    for r in range(view.size(0)):                           # row by row, through slices
        view[r:r + 1].copy_(small[r:r + 1])


def _inputs(kind, bits):
    """(a, weight operands (tuple), truth float64 [M, N]) on the device, compact"""
    rng = np.random.default_rng([KINDS.index(kind), 0xFA7])
    dt = TDT[bits]
    if kind == "mxfp4":
        a64, packed, scale, _ = mxfp4_ref.int_inputs(rng, M, K, N, False)
        truth = mxfp4_ref.mxfp4_ref(a64, packed, scale)
        w = (torch.as_tensor(packed).to(DEV), scale.to(DEV))
    else:
        a64, w64, _ = dense_ref.int_inputs(rng, M, K, N, False)
        truth = a64 @ w64.T
        wt = torch.from_numpy(w64).to(DEV)
        w = (wt.to(dt),)
        if kind == "fp8":                                   # power-of-two column scales: every product stays exact
            sc = 2.0 ** rng.integers(-1, 2, size=(N,))
            w, truth = (wt.float().to(torch.float8_e4m3fn), torch.from_numpy(sc).float().to(DEV)), truth * sc[None, :]
    return torch.from_numpy(a64).to(DEV).to(dt), w, truth


def _launch(kind, a, w, c):
    from scalellm_amd import kernels
    if kind == "dense":
        plan = kernels.linear_plan(a, w[0], c)
        kernels.linear(a, w[0], c)
    elif kind == "fp8":
        plan = kernels.fp8_linear_plan(a, w[0], w[1], c)
        kernels.fp8_linear(a, w[0], w[1], c)
    else:
        plan = kernels.mxfp4_linear_plan(a, w[0], w[1], c)
        kernels.mxfp4_linear(a, w[0], w[1], c)
    torch.cuda.synchronize()
    return (plan.row_tiles, plan.waves, plan.row_blocks, plan.col_groups, plan.split_k, plan.n_chunks)


@pytest.mark.parametrize("split", (1, 3))
@pytest.mark.parametrize("far", FAR)
@pytest.mark.parametrize("bits", ref.BITS)
@pytest.mark.parametrize("kind", KINDS)
def test_far_linear(kind, bits, far, split, tune, arena):
    tune(SLM_LINEAR_SPLITK=split)
    dt = TDT[bits]
    a, w, truth = _inputs(kind, bits)
    c_near = torch.full((M, N), float("nan"), dtype=dt, device=DEV)
    plan_near = _launch(kind, a, w, c_near)
    assert plan_near[4] == split
    F.refill(arena, bits)
    a_far, w_far, c_far, written = a, w, torch.full((M, N), float("nan"), dtype=dt, device=DEV), []
    if far == "A":
        a_far, written = _far_view(arena, dt, M, K)
        _put(a_far, a)
    elif far == "C":
        c_far, written = _far_view(arena, dt, M, N)
    else:
        w0, written = _far_view(arena, w[0].dtype, N, w[0].size(1))
        _put(w0, w[0])
        w_far = (w0,) + tuple(w[1:])
        if kind == "mxfp4":                                 # the block scales ride along, in region V
            s0, more = _far_view(arena, torch.uint8, N, K // 32, base=F.V_BASE)
            _put(s0, w[1])
            w_far, written = (w0, s0), written + more
    far_op = {"A": a_far, "W": w_far[0], "C": c_far}[far]
    assert (far_op.size(0) - 1) * far_op.stride(0) * far_op.element_size() >= 2 ** 32
    plan_far = _launch(kind, a_far, w_far, c_far)
    assert plan_far == plan_near, "the strides must not change the plan"
    assert F.untouched(arena, written, bits), "wrote the arena outside the far operand's rows"
    got = np.stack([_bits(c_far[r:r + 1])[0] for r in range(M)])
    assert np.array_equal(got, _bits(c_near)), (kind, bits, far, split, "differs from the compact call")
    assert np.array_equal(got, ref.f64_to_t_bits(truth, bits)), (kind, bits, far, split, "differs from the integer truth")


@pytest.mark.parametrize("bits", ref.BITS)
@pytest.mark.parametrize("far,m,k,n", [("A", 33, 1024, 512), ("C", 33, 1024, 512), ("A", 129, 512, 14336)])
def test_far_int4_gemm(far, m, k, n, bits, arena):
    from scalellm_amd import kernels
    dt = TDT[bits]
    case = w4._c(m, n, k, 128, "gptq")
    q, a_np, _, truth, _ = w4.inputs(bits, case)
    a = torch.from_numpy(np.ascontiguousarray(a_np)).to(DEV).to(dt)
    packed = helpers.pack_case(q, bits)
    near, plan_a, plan_c = W4_FAR_PLANS[(m, k, n)]
    c_near = torch.full((m, n), float("nan"), dtype=dt, device=DEV)
    info = kernels.w4_plan(a, packed, c_near)
    assert (info.kernel_name, info.row_tiles) == near
    kernels.gptq_gemm(a, packed, c_near)
    F.refill(arena, bits)
    a_far, c_far, written = a, torch.full((m, n), float("nan"), dtype=dt, device=DEV), []
    if far == "A":
        a_far, written = _far_view(arena, dt, m, k)
        _put(a_far, a)
    else:
        c_far, written = _far_view(arena, dt, m, n)
    info = kernels.w4_plan(a_far, packed, c_far)
    assert (info.kernel_name, info.row_tiles) == (plan_a if far == "A" else plan_c), "the fall-back the CPU test named"
    kernels.gptq_gemm(a_far, packed, c_far)
    torch.cuda.synchronize()
    assert F.untouched(arena, written, bits), "wrote the arena outside the far operand's rows"
    got = np.stack([_bits(c_far[r:r + 1])[0] for r in range(m)])
    assert np.array_equal(got, _bits(c_near)), (far, m, bits, "differs from the compact call")
    helpers.assert_bits_equal(c_near, truth, dt, f"int4 compact {m} x {k} x {n} {bits}")


MOE_T, MOE_E, MOE_N = F.MOE_T, F.MOE_E, F.MOE_N         # N / 2 a multiple of 32 for the SiLU.mul form


def _moe_inputs(kind, bits):
    """(a [T, K] of T, weight stack, scale stack or None, expert id per token int32 [T, 1], truth float64 [T, N])"""
    rng = np.random.default_rng([KINDS.index(kind), 0xE0E])
    dt = TDT[bits]
    a64 = rng.integers(-4, 5, size=(MOE_T, K)).astype(np.float64)
    if kind == "mxfp4":
        per = [mxfp4_ref.int_inputs(rng, 1, K, MOE_N, False)[1:3] for _ in range(MOE_E)]
        w = torch.stack([torch.as_tensor(p) for p, _ in per]).to(DEV)
        scale = torch.stack([sc for _, sc in per]).to(DEV)
        w64 = np.stack([mxfp4_ref.w_as64(p, sc) for p, sc in per])
    else:
        wi = rng.integers(-4, 5, size=(MOE_E, MOE_N, K)).astype(np.float64)
        if kind == "fp8":                                   # power-of-two column scales: every product stays exact
            sc = 2.0 ** rng.integers(-1, 2, size=(MOE_E, MOE_N))
            w, scale, w64 = torch.from_numpy(wi).float().to(DEV).to(torch.float8_e4m3fn), \
                torch.from_numpy(sc).float().to(DEV), wi * sc[:, :, None]
        else:
            w, scale, w64 = torch.from_numpy(wi).to(DEV).to(dt), None, wi
    ids = rng.integers(0, MOE_E, size=(MOE_T, 1))
    ids[:3, 0] = [0, 1, 2]                                    # every expert has a token
    truth = np.einsum("tk,tnk->tn", a64, w64[ids[:, 0]])
    return torch.from_numpy(a64).to(DEV).to(dt), w, scale, ids.astype(np.int32), truth


def _far_stack(arena, small, base, layout):
    """(view of the arena shaped like the stack `small` [E, ...] with a far expert stride, holding its values; the
    element ranges (int16 units) it covers).  layout "past": far_ld (expert 1 past 2^31, expert 2 past 2^32, every alias
    poison); "across": across_stride (offsets inside expert 1 cross 2^31, inside expert 2 cross 2^32)."""
    es = small.element_size()
    block = small[0].numel()
    stride = F.far_ld(MOE_E, es) if layout == "past" else F.across_stride(block * es, es)
    flat = arena.view(small.dtype)
    v = torch.as_strided(flat, tuple(small.shape), (stride,) + tuple(small.stride()[1:]), storage_offset=base // es)
    spans = []
    for e in range(MOE_E):
        v[e:e + 1].copy_(small[e:e + 1])
        lo = base + e * stride * es
        spans.append((lo // 2, (lo + block * es + 1) // 2))
    assert (MOE_E - 1) * stride * es + block * es > 2 ** 32 and stride * es + block * es > 2 ** 31
    return v, spans


@pytest.mark.parametrize("silu", (False, True))
@pytest.mark.parametrize("far", ("experts past", "experts across", "A", "C"))
@pytest.mark.parametrize("bits", ref.BITS)
@pytest.mark.parametrize("kind", KINDS)
def test_far_moe_gemm(kind, bits, far, silu, arena):
    from scalellm_amd import kernels
    dt = TDT[bits]
    a, w, scale, ids, truth = _moe_inputs(kind, bits)
    cap, blocks = kernels.moe_align_capacity(MOE_T, MOE_E, 32)
    sorted_idx = torch.empty(cap, dtype=torch.int32, device=DEV)
    expert_ids = torch.empty(blocks, dtype=torch.int32, device=DEV)
    n_padded = torch.empty(1, dtype=torch.int32, device=DEV)
    kernels.moe_align_block(torch.from_numpy(ids).to(DEV), MOE_E, 32, sorted_idx, expert_ids, n_padded)
    n_out = MOE_N // 2 if silu else MOE_N

    def run(a_, w_, s_, c_):
        tail = (c_, sorted_idx, expert_ids, n_padded, 1)
        if kind == "dense":
            kernels.moe_grouped_gemm(a_, w_, *tail, silu_mul=silu)
        elif kind == "fp8":
            kernels.moe_fp8_grouped_gemm(a_, w_, s_, *tail, silu_mul=silu)
        else:
            kernels.moe_mxfp4_grouped_gemm(a_, w_, s_, *tail, silu_mul=silu)
        torch.cuda.synchronize()

    c_near = torch.full((MOE_T, n_out), float("nan"), dtype=dt, device=DEV)
    run(a, w, scale, c_near)
    F.refill(arena, bits)
    a_far, w_far, s_far, written = a, w, scale, []
    c_far = torch.full((MOE_T, n_out), float("nan"), dtype=dt, device=DEV)
    if far == "A":
        a_far, written = _far_view(arena, dt, MOE_T, K)
        _put(a_far, a)
    elif far == "C":
        c_far, written = _far_view(arena, dt, MOE_T, n_out)
    else:                                                   # the weights in region K, their scales in region V
        w_far, written = _far_stack(arena, w, F.K_BASE, far.split()[1])
        if scale is not None:
            s_far, more = _far_stack(arena, scale, F.V_BASE, far.split()[1])
            written = written + more
    run(a_far, w_far, s_far, c_far)
    assert F.untouched(arena, written, bits), "wrote the arena outside the far operand's rows"
    got = np.stack([_bits(c_far[r:r + 1])[0] for r in range(MOE_T)])
    assert np.array_equal(got, _bits(c_near)), (kind, bits, far, silu, "differs from the compact call")
    if not silu:
        assert np.array_equal(got, ref.f64_to_t_bits(truth, bits)), (kind, bits, far, "differs from the integer truth")
