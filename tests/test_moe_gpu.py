"""GPU tests of the mixture-of-experts path (include/slm_hip.h section 10) against tests/moe_ref.py and, for the
grouped GEMM, against the per-expert dequantised weights (kernels.w4_dequant, pinned bit-exact by test_w4_gpu) and
an fp32 matmul scattered as the reference's grouped_gemm_ref does (src/kernels/gemm/sm80_grouped_gemm_test.cu).
Grids follow the reference's own tests: topk_softmax_kernel_test.cu, grouped_topk_sigmoid_kernel_test.cu,
align_block_kernel_test.cu."""
import numpy as np
import pytest
import torch

from tests import helpers

from . import moe_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEMM_TOL = {"f16": 1e-3, "bf16": 8e-3}   # tests/test_w4_gpu.py:90-94


def _rel_err(c, r):
    return float(np.abs(c - r).mean() / np.abs(r).mean())


def _dt(bits):
    return torch.bfloat16 if bits == "bf16" else torch.float16


# ---- routing -----------------------------------------------------------------------------------------
def test_topk_softmax_reference_grid():
    from scalellm_amd import kernels
    rng = np.random.default_rng(2024)
    for T in (1, 10, 16, 128, 1024):
        for E in (4, 8, 16, 32, 64, 128, 256):
            x = rng.standard_normal((T, E)).astype(np.float32) * 2.0
            xd = torch.from_numpy(x).to(DEV)
            for k in (1, 2, 4):
                if k > E:
                    continue
                w, i = kernels.moe_topk_softmax(xd, k)
                rw, ri = ref.topk_softmax(x, k)
                assert np.array_equal(i.cpu().numpy(), ri), (T, E, k)
                np.testing.assert_allclose(w.cpu().numpy().astype(np.float64), rw, rtol=1e-5, atol=1e-8)


def test_topk_softmax_ties_renormalize_and_large_k():
    from scalellm_amd import kernels
    rng = np.random.default_rng(7)
    # duplicated logits: few distinct values, so every row has ties at the cut (and -0 / +0)
    x = rng.integers(-2, 3, size=(37, 64)).astype(np.float32)
    x[x == 0] *= rng.choice([-1.0, 1.0], size=int((x == 0).sum())).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    for k in (1, 2, 4, 8):
        w, i = kernels.moe_topk_softmax(xd, k)
        rw, ri = ref.topk_softmax(x, k)
        assert np.array_equal(i.cpu().numpy(), ri), k
        np.testing.assert_allclose(w.cpu().numpy().astype(np.float64), rw, rtol=1e-5, atol=1e-8)
    y = rng.standard_normal((33, 8)).astype(np.float32)
    w, i = kernels.moe_topk_softmax(torch.from_numpy(y).to(DEV), 2, renormalize=True)
    rw, ri = ref.topk_softmax(y, 2, renormalize=True)
    assert np.array_equal(i.cpu().numpy(), ri)
    np.testing.assert_allclose(w.cpu().numpy().astype(np.float64), rw, rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(w.sum(dim=1).cpu().numpy(), 1.0, rtol=1e-6)
    # k = E > 64: every output slot of every lane; a full descending sort
    z = rng.standard_normal((3, 256)).astype(np.float32)
    w, i = kernels.moe_topk_softmax(torch.from_numpy(z).to(DEV), 256)
    rw, ri = ref.topk_softmax(z, 256)
    assert np.array_equal(i.cpu().numpy(), ri)
    np.testing.assert_allclose(w.cpu().numpy().astype(np.float64), rw, rtol=1e-5, atol=1e-8)
    # bit-identical repeats
    w2, i2 = kernels.moe_topk_softmax(torch.from_numpy(z).to(DEV), 256)
    assert torch.equal(w, w2) and torch.equal(i, i2)


def test_grouped_topk_sigmoid_reference_grid():
    from scalellm_amd import kernels
    n_tokens = n_skipped = 0
    for E in (128, 256):
        for k in (1, 2, 8):
            for T in (1, 10, 64):
                rng = np.random.default_rng(1000 + E + k + T)
                x = rng.standard_normal((T, E)).astype(np.float32)
                bias = rng.standard_normal(E).astype(np.float32)
                w, i = kernels.moe_grouped_topk_sigmoid(torch.from_numpy(x).to(DEV), torch.from_numpy(bias).to(DEV),
                                                        8, 4, k, 2.5)
                rw, ri, margin = ref.grouped_topk_sigmoid(x, bias, 8, 4, k, 2.5, with_margin=True)
                clear = margin > 1e-5
                n_tokens += T
                n_skipped += int((~clear).sum())
                assert np.array_equal(i.cpu().numpy()[clear], ri[clear]), (E, k, T)
                np.testing.assert_allclose(w.cpu().numpy().astype(np.float64)[clear], rw[clear], rtol=1e-5, atol=1e-8)
    assert n_skipped <= 0.02 * n_tokens, (n_skipped, n_tokens)


def test_grouped_topk_sigmoid_group_rule_and_ties():
    """the hand-worked case of test_moe_cpu on the device: group selection by the top-2 sum, ties to the lower index
    (experts and groups), weights from the unbiased sigmoid"""
    from scalellm_amd import kernels
    x = torch.zeros(2, 8, device=DEV)
    bias = torch.tensor([0.375, -0.5, 0.125, 0.125, 0.25, 0.0, 0.0, 0.0625], device=DEV)
    w, i = kernels.moe_grouped_topk_sigmoid(x, bias, 4, 2, 3, 2.5)
    assert i.tolist() == [[4, 2, 3]] * 2 and w.tolist() == [[1.25] * 3] * 2
    w, i = kernels.moe_grouped_topk_sigmoid(x, bias, 4, 1, 2, 1.0)
    assert i.tolist() == [[2, 3]] * 2


# ---- align -------------------------------------------------------------------------------------------
SENTINEL, GUARD = -77, 64


def _check_align(ids_np, E, block):
    from scalellm_amd import kernels
    n_flat = ids_np.size
    cap, blocks = kernels.moe_align_capacity(n_flat, E, block)
    srt = torch.full((cap + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    eid = torch.full((blocks + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    npad = torch.full((1 + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    cu = torch.full((E + 1 + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    kernels.moe_align_block(torch.from_numpy(ids_np).to(DEV), E, block, srt[:cap], eid[:blocks], npad[:1], cu[:E + 1])
    rs, re_, rn, rcu = ref.align_block(ids_np, E, block)
    what = (ids_np.shape, E, block)
    assert int(npad[0]) == rn and rn <= cap, what
    assert np.array_equal(srt[:rn].cpu().numpy(), rs), what          # [0, n_padded) fully written, padding included
    assert np.array_equal(eid[:rn // block].cpu().numpy(), re_), what
    assert np.array_equal(cu[:E + 1].cpu().numpy(), rcu), what
    for buf, used in ((srt, cap), (eid, blocks), (npad, 1), (cu, E + 1)):
        assert bool((buf[used:] == SENTINEL).all()), what             # the guard region is untouched


@pytest.mark.parametrize("E", [8, 64, 256])
def test_align_block_reference_grid(E):
    rng = np.random.default_rng(300 + E)
    for T in (1, 2, 33, 256, 1024):
        for k in (1, 2, 8):
            ids = rng.integers(0, E, size=(T, k)).astype(np.int32)
            for block in (16, 32, 64, 128):
                if T == 1024 and block in (64, 128) and k != 8:       # thinned; T * k > 1024 and E > 64 stay covered
                    continue
                _check_align(ids, E, block)


def test_align_block_adversarial_assignments():
    for T, k, E in ((1, 1, 8), (3, 2, 8), (5, 8, 256), (33, 2, 8), (64, 1, 64), (256, 8, 8), (1024, 2, 1024), (7, 8, 64)):
        for ids in ref.adversarial_assignments(T, k, E).values():
            for block in (16, 32, 256):
                _check_align(ids, E, block)


def test_align_block_is_reproducible_and_drops_foreign_ids():
    from scalellm_amd import kernels
    rng = np.random.default_rng(5)
    ids = rng.integers(-1, 9, size=(300, 4)).astype(np.int32)        # -1 and 8 are not experts of E = 8
    _check_align(ids, 8, 32)
    cap, blocks = kernels.moe_align_capacity(ids.size, 8, 32)
    outs = []
    for _ in range(2):
        srt = torch.zeros(cap, dtype=torch.int32, device=DEV)
        eid = torch.zeros(blocks, dtype=torch.int32, device=DEV)
        npad = torch.zeros(1, dtype=torch.int32, device=DEV)
        kernels.moe_align_block(torch.from_numpy(ids).to(DEV), 8, 32, srt, eid, npad)
        outs.append((srt[:int(npad[0])].clone(), eid[:int(npad[0]) // 32].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- sum ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_moe_sum(bits):
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(3)
    for T, k, dim in ((1, 1, 8), (3, 2, 256), (5, 3, 4104), (2, 8, 100), (70, 5, 136), (4, 7, 3)):
        x = torch.randn(T, k, dim, device=DEV, dtype=_dt(bits), generator=g)
        full = torch.full((T + 1, dim), float("nan"), device=DEV, dtype=_dt(bits))
        kernels.moe_sum(x, full[:T])
        acc = torch.zeros(T, dim, device=DEV, dtype=torch.float32)
        for j in range(k):                                            # fp32, in order j = 0..k-1, one rounding
            acc = acc + x[:, j].float()
        assert torch.equal(full[:T], acc.to(_dt(bits))), (T, k, dim)
        assert bool(torch.isnan(full[T]).all())


# ---- grouped GEMM ------------------------------------------------------------------------------------
def _experts(seed, E, K, N, gs, fmt, bits, paired=False):
    """E random experts: (PackedMoeW4, [E] fp32 dense weights [K, N] from w4_dequant, in checkpoint column order)"""
    from scalellm_amd import _lib, kernels
    cases = [helpers.make_quant_case(seed * 1000 + e, K, N, gs, fmt, bits) for e in range(E)]
    code = _lib.SLM_W4_AWQ if fmt == "awq" else _lib.SLM_W4_GPTQ
    plain = [helpers.pack_case(c, bits) for c in cases]
    dense = [kernels.w4_dequant(p).float().cpu().numpy() for p in plain]
    stacked = kernels.moe_stack_experts([helpers.pack_case(c, bits, paired=True) for c in cases] if paired else plain,
                                        code)
    return stacked, dense, kernels.moe_stack_experts(plain, code)


def _routing(rng, T, k, E):
    return np.stack([rng.permutation(E)[:k] for _ in range(T)]).astype(np.int32)


def _aligned(ids_np, E):
    """the aligned block list of moe_ref in buffers of the capacity size (entries past n_padded hold the padding
    id: blocks beyond n_padded must not be computed, and could store nothing if they were)"""
    from scalellm_amd import kernels
    cap, blocks = kernels.moe_align_capacity(ids_np.size, E, 32)
    rs, re_, rn, _ = ref.align_block(ids_np, E, 32)
    srt = np.full(cap, ids_np.size, np.int32)
    eid = np.zeros(blocks, np.int32)
    srt[:rn], eid[:rn // 32] = rs, re_
    return (torch.from_numpy(srt).to(DEV), torch.from_numpy(eid).to(DEV),
            torch.tensor([rn], dtype=torch.int32, device=DEV))


def _grouped_ref(a_np, dense, ids_np, a_div):
    flat = ids_np.reshape(-1)
    out = np.zeros((flat.size, dense[0].shape[1]), np.float32)
    for f, e in enumerate(flat):
        out[f] = a_np[f // a_div] @ dense[e]
    return out


def _gemm_cases():
    cases, i = [], 0
    for K in (128, 384, 640):
        for N in (64, 128, 320):
            for E in (1, 8, 64):
                for T in (1, 3, 33, 96):
                    for k in (1, 2, 4):
                        for gs in (32, 64, 128, -1):
                            i += 1
                            if k > E or i % 43 != 0:                      # thin the product
                                continue
                            cases.append((K, N, E, T, k, gs))
    return cases


GEMM_CASES = _gemm_cases()


def test_gemm_case_list_covers_every_axis():
    assert 20 <= len(GEMM_CASES) <= 30          # x 2 formats x 2 dtypes: roughly 100 cases
    for axis, want in enumerate(((128, 384, 640), (64, 128, 320), (1, 8, 64), (1, 3, 33, 96), (1, 2, 4),
                                 (32, 64, 128, -1))):
        assert {c[axis] for c in GEMM_CASES} == set(want), axis


@pytest.mark.parametrize("fmt", ["awq", "gptq"])
@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_grouped_gemm_grid(bits, fmt):
    from scalellm_amd import kernels
    dt = _dt(bits)
    for n, (K, N, E, T, k, gs) in enumerate(GEMM_CASES):
        rng = np.random.default_rng(n)
        g = torch.Generator(device=DEV).manual_seed(n)
        experts, dense, _ = _experts(n + (50 if fmt == "awq" else 0), E, K, N, gs, fmt, bits)
        ids = _routing(rng, T, k, E)
        srt, eid, npad = _aligned(ids, E)
        a_div = k if n % 2 == 0 else 1                               # the token matrix, or one row per (token, expert)
        a = torch.randn(T * k // a_div, K, device=DEV, dtype=dt, generator=g)
        full = torch.full((T * k + 1, N), float("nan"), device=DEV, dtype=dt)
        kernels.moe_w4_grouped_gemm(a, experts, full[:T * k], srt, eid, npad, a_div)
        out = full[:T * k].float().cpu().numpy()
        what = (K, N, E, T, k, gs, a_div)
        assert not np.isnan(out).any(), what                         # every row of [T * k] is written
        assert bool(torch.isnan(full[T * k]).all()), what            # the guard row is not
        err = _rel_err(out, _grouped_ref(a.float().cpu().numpy(), dense, ids, a_div))
        assert err < GEMM_TOL[bits], (what, err)
        again = torch.full((T * k, N), float("nan"), device=DEV, dtype=dt)
        kernels.moe_w4_grouped_gemm(a, experts, again, srt, eid, npad, a_div)
        assert torch.equal(again, full[:T * k]), what                # two runs: bit-identical


@pytest.mark.parametrize("bits", ["bf16", "f16"])
@pytest.mark.parametrize("K,N,E,T,k,gs,fmt", [(128, 64, 1, 3, 1, 128, "awq"), (384, 128, 8, 33, 2, 32, "gptq"),
                                              (640, 320, 8, 96, 4, 64, "awq"), (384, 640, 64, 33, 4, -1, "gptq"),
                                              (256, 192, 8, 1, 2, 128, "awq")])
def test_grouped_gemm_silu_mul_is_bit_identical_to_the_unfused_sequence(bits, K, N, E, T, k, gs, fmt):
    from scalellm_amd import kernels
    dt = _dt(bits)
    rng = np.random.default_rng(K + N + E + T)
    g = torch.Generator(device=DEV).manual_seed(K + T)
    paired, dense, plain = _experts(900 + K + N, E, K, N, gs, fmt, bits, paired=True)
    ids = _routing(rng, T, k, E)
    srt, eid, npad = _aligned(ids, E)
    a = torch.randn(T, K, device=DEV, dtype=dt, generator=g)
    n_flat = T * k
    unfused = torch.empty(n_flat, N, device=DEV, dtype=dt)
    kernels.moe_w4_grouped_gemm(a, plain, unfused, srt, eid, npad, k)
    want = torch.empty(n_flat, N // 2, device=DEV, dtype=dt)
    kernels.silu_and_mul(want, unfused)
    full = torch.full((n_flat + 1, N // 2), float("nan"), device=DEV, dtype=dt)
    kernels.moe_w4_grouped_gemm(a, paired, full[:n_flat], srt, eid, npad, k, silu_mul=True)
    assert torch.equal(full[:n_flat], want)
    assert bool(torch.isnan(full[n_flat]).all())
    # ... and it is the right function: silu(gate) * up of the fp32 reference at the GEMM tolerance
    r = _grouped_ref(a.float().cpu().numpy(), dense, ids, k).astype(np.float64)
    gate, up = r[:, :N // 2], r[:, N // 2:]
    err = _rel_err(full[:n_flat].float().cpu().numpy(), gate / (1 + np.exp(-gate)) * up)
    assert err < 2 * GEMM_TOL[bits], err   # two GEMM outputs meet in one product


@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_grouped_gemm_row_scale(bits):
    from scalellm_amd import kernels
    dt = _dt(bits)
    for n, (K, N, E, T, k, gs, fmt) in enumerate([(384, 128, 8, 33, 2, 128, "awq"), (128, 320, 64, 96, 4, 32, "gptq"),
                                                  (640, 64, 8, 3, 2, -1, "gptq")]):
        rng = np.random.default_rng(40 + n)
        g = torch.Generator(device=DEV).manual_seed(40 + n)
        experts, dense, _ = _experts(700 + n, E, K, N, gs, fmt, bits)
        ids = _routing(rng, T, k, E)
        srt, eid, npad = _aligned(ids, E)
        a = torch.randn(T * k, K, device=DEV, dtype=dt, generator=g)
        w = torch.rand(T * k, device=DEV, generator=g) + 0.05
        out = torch.full((T * k, N), float("nan"), device=DEV, dtype=dt)
        kernels.moe_w4_grouped_gemm(a, experts, out, srt, eid, npad, 1, row_scale=w)
        want = w.cpu().numpy()[:, None] * _grouped_ref(a.float().cpu().numpy(), dense, ids, 1)
        o = out.float().cpu().numpy()
        assert not np.isnan(o).any()
        assert _rel_err(o, want) < GEMM_TOL[bits]


# The grouped kernel and the dense lean kernel (w4_small.hip) run one main loop (csrc/w4_stream32.h): the same
# arithmetic in the same order, so they agree bit for bit.  (rows of expert 0, rows of expert 1, K, N, group, silu);
# every expert has >= 2 rows: M = 1 plans the GEMV.
STREAM_CASES = [
    (17, 5, 256, 192, 128, False),    # two chunks < the ring of four; the last workgroup: two valid, two clamped waves
    (32, 2, 640, 64, 32, False),      # five chunks, four scale groups per chunk
    (9, 31, 640, 128, 64, False),     # two scale groups per chunk
    (3, 20, 1024, 64, 256, False),    # groups spanning chunks
    (6, 11, 384, 64, 384, False),     # per-channel, K no power of two
    (8, 12, 256, 128, 128, True),     # paired experts, SiLU*mul epilogue on both sides
]


@pytest.mark.parametrize("bits", ["bf16", "f16"])
@pytest.mark.parametrize("n", range(len(STREAM_CASES)))
def test_grouped_gemm_is_bit_identical_to_the_dense_lean_kernel(n, bits):
    from scalellm_amd import _lib, kernels
    r0, r1, K, N, gs, silu = STREAM_CASES[n]
    fmt = ("awq", "gptq")[(n + (bits == "f16")) % 2]                 # alternating; each case sees both over the dtypes
    dt, T = _dt(bits), r0 + r1
    packed = [helpers.pack_case(helpers.make_quant_case(7000 + 10 * n + e, K, N, gs, fmt, bits), bits, paired=silu)
              for e in range(2)]
    experts = kernels.moe_stack_experts(packed, _lib.SLM_W4_AWQ if fmt == "awq" else _lib.SLM_W4_GPTQ)
    # top-1 routing by hand: expert 1 takes r1 tokens spread over the batch, so both experts gather
    assert np.gcd(7, T) == 1
    ids = np.array([0] * r0 + [1] * r1, np.int32)[(np.arange(T) * 7) % T]
    cap, blocks = kernels.moe_align_capacity(T, 2, 32)
    srt = torch.empty(cap, dtype=torch.int32, device=DEV)
    eid = torch.empty(blocks, dtype=torch.int32, device=DEV)
    npad = torch.empty(1, dtype=torch.int32, device=DEV)
    kernels.moe_align_block(torch.from_numpy(ids).to(DEV), 2, 32, srt, eid, npad)
    g = torch.Generator(device=DEV).manual_seed(n)
    a = torch.randn(T, K, device=DEV, dtype=dt, generator=g)
    n_out = N // 2 if silu else N
    out = torch.full((T, n_out), float("nan"), device=DEV, dtype=dt)
    kernels.moe_w4_grouped_gemm(a, experts, out, srt, eid, npad, 1, silu_mul=silu)
    for e, rows in enumerate((r0, r1)):
        idx = torch.from_numpy(np.nonzero(ids == e)[0]).to(DEV)
        assert idx.numel() == rows
        a_e = a[idx].contiguous()
        want = torch.full((rows, n_out), float("nan"), device=DEV, dtype=dt)
        with kernels.tuning(SLM_W4_KS=0, SLM_W4_SPLITK=1):
            assert kernels.w4_plan(a_e, experts.expert(e), want, silu_mul=silu).kernel_name == "SMALL"
            kernels.gptq_gemm(a_e, experts.expert(e), want, silu_mul=silu)
        assert not bool(torch.isnan(want).any())
        assert torch.equal(out[idx], want), (STREAM_CASES[n], fmt, e)


# ---- FusedMoE end to end -----------------------------------------------------------------------------
HID, INTER, NE, TOPK = 256, 384, 8, 2


def _moe_layer(bits, scoring, fmt="awq", gs=128, max_tokens=70, seed=0):
    from scalellm_amd import kernels, moe
    from scalellm_amd.layers import QuantArgs
    dt = _dt(bits)
    sd, dense = {}, {}
    for e in range(NE):
        for w, (K, N) in (("w1", (HID, INTER)), ("w3", (HID, INTER)), ("w2", (INTER, HID))):
            c = helpers.make_quant_case(seed * 100 + e * 3 + len(sd), K, N, gs, fmt, bits)
            sd[f"experts.{e}.{w}.qweight"] = torch.from_numpy(c["qweight"])
            sd[f"experts.{e}.{w}.qzeros"] = torch.from_numpy(c["qzeros"])
            sd[f"experts.{e}.{w}.scales"] = torch.from_numpy(c["scales_bits"].view(np.int16)).view(dt)
            dense[(e, w)] = kernels.w4_dequant(helpers.pack_case(c, bits)).float()
    g = torch.Generator().manual_seed(seed)
    sd["gate.weight"] = (torch.randn(NE, HID, generator=g) * 0.5).to(dt)
    sd["gate.e_score_correction_bias"] = torch.randn(NE, generator=g) * 0.1
    layer = moe.FusedMoE(HID, INTER, NE, TOPK, QuantArgs(fmt, 4, gs), scoring=scoring, renormalize=True,
                         n_expert_groups=4, topk_group=2, scaling_factor=1.5, max_tokens=max_tokens, dtype=dt, device=DEV)
    layer.load_state_dict(sd)
    return layer, dense


def _moe_reference(layer, dense, x):
    """torch fp32 composition rounding to T after SiLU * mul, after the row scale and after the sum"""
    dt = x.dtype
    logits = (x.float() @ layer.gate_weight.float().t()).cpu().numpy()
    if layer.scoring == "softmax":
        w, ids = ref.topk_softmax(logits, TOPK, renormalize=True)
    else:
        w, ids = ref.grouped_topk_sigmoid(logits, layer.correction_bias.cpu().numpy(), 4, 2, TOPK, 1.5)
    out = torch.zeros(x.size(0), HID, device=DEV, dtype=torch.float32)
    for t in range(x.size(0)):
        acc = torch.zeros(HID, device=DEV, dtype=torch.float32)
        for j in range(TOPK):
            e = int(ids[t, j])
            gate, up = x[t].float() @ dense[(e, "w1")], x[t].float() @ dense[(e, "w3")]
            act = (torch.nn.functional.silu(gate) * up).to(dt)
            acc = acc + (float(w[t, j]) * (act.float() @ dense[(e, "w2")])).to(dt).float()
        out[t] = acc
    return out.to(dt)


@pytest.mark.parametrize("scoring", ["softmax", "grouped_sigmoid"])
@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_fused_moe_end_to_end(bits, scoring):
    layer, dense = _moe_layer(bits, scoring, fmt="awq" if bits == "bf16" else "gptq")
    g = torch.Generator(device=DEV).manual_seed(11)
    for T in (1, 5, 70):
        x = torch.randn(T, HID, device=DEV, dtype=_dt(bits), generator=g)
        y = layer(x)
        want = _moe_reference(layer, dense, x)
        assert y.shape == x.shape and not bool(torch.isnan(y).any())
        err = _rel_err(y.float().cpu().numpy(), want.float().cpu().numpy())
        assert err < 2 * GEMM_TOL[bits], (T, err)      # two chained GEMMs, GEMM_TOL each
        assert torch.equal(layer(x), y)                # bit-identical repeats


@pytest.mark.parametrize("scoring", ["softmax", "grouped_sigmoid"])
def test_fused_moe_graph_replay_matches_eager(scoring):
    T = 5
    layer, _ = _moe_layer("bf16", scoring, max_tokens=T)
    g = torch.Generator(device=DEV).manual_seed(21)
    xs = [torch.randn(T, HID, device=DEV, dtype=torch.bfloat16, generator=g) for _ in range(3)]
    xs.append(xs[0][:1].expand(T, HID).contiguous())               # every token to the same two experts
    eager, padded = [], []
    for x in xs:
        eager.append(layer(x).clone())
        padded.append(int(layer._buf["n_padded"][0]))
    assert padded[-1] == 64 and len(set(padded)) >= 2              # the replays see different padded counts
    x_static = xs[0].clone()
    out_static = torch.empty_like(x_static)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer.forward(x_static, out=out_static)
    for x, want in zip(xs, eager):
        x_static.copy_(x)
        graph.replay()
        assert torch.equal(out_static, want)
    torch.cuda.synchronize()


# ---- the C++ shim --------------------------------------------------------------------------------------
def test_shim_functions_match_the_ctypes_path():
    from scalellm_amd import kernels
    from scalellm_amd.cpp_host import load_shim
    shim = load_shim()
    rng = np.random.default_rng(9)
    T, E, k = 33, 64, 4
    x = torch.from_numpy(rng.standard_normal((T, E)).astype(np.float32)).to(DEV)
    bias = torch.from_numpy(rng.standard_normal(E).astype(np.float32)).to(DEV)
    w, i = kernels.moe_topk_softmax(x, k)
    w2, i2 = torch.empty_like(w), torch.empty_like(i)
    shim.moe_topk_softmax(x, w2, i2)
    assert torch.equal(w, w2) and torch.equal(i, i2)
    wr, ir = kernels.moe_topk_softmax(x, k, renormalize=True)
    shim.moe_topk_softmax_renorm(x, w2, i2)
    assert torch.equal(wr, w2) and torch.equal(ir, i2)
    wg, ig = kernels.moe_grouped_topk_sigmoid(x, bias, 8, 4, k, 2.5)
    shim.moe_grouped_topk_sigmoid(x, bias, 8, 4, k, 2.5, w2, i2)
    assert torch.equal(wg, w2) and torch.equal(ig, i2)

    cap, blocks = kernels.moe_align_capacity(T * k, E, 32)
    bufs = [[torch.zeros(n, dtype=torch.int32, device=DEV) for n in (cap, blocks, 1, E + 1)] for _ in range(2)]
    kernels.moe_align_block(i, E, 32, *bufs[0])
    shim.moe_permute_align_block(i, E, 32, *bufs[1])
    n = int(bufs[0][2][0])
    assert n == int(bufs[1][2][0]) and torch.equal(bufs[0][0][:n], bufs[1][0][:n])
    assert torch.equal(bufs[0][1][:n // 32], bufs[1][1][:n // 32]) and torch.equal(bufs[0][3], bufs[1][3])
    srt, eid, npad, _ = bufs[0]

    K, N = 256, 128
    paired, _, plain = _experts(77, E, K, N, 64, "awq", "bf16", paired=True)
    a = torch.randn(T, K, device=DEV, dtype=torch.bfloat16)
    for experts, silu, scale in ((plain, False, None), (plain, False, w.reshape(-1).contiguous()), (paired, True, None)):
        n_out = N // 2 if silu else N
        c1 = torch.zeros(T * k, n_out, device=DEV, dtype=torch.bfloat16)
        c2 = torch.zeros_like(c1)
        kernels.moe_w4_grouped_gemm(a, experts, c1, srt, eid, npad, k, row_scale=scale, silu_mul=silu)
        fmt = experts.fmt | (0x10 if experts.paired else 0)
        shim.moe_w4_grouped_gemm(a, experts.wq, experts.sz, c2, srt, eid, npad, K, N, 64, k, fmt, scale, silu)
        assert torch.equal(c1, c2)
    y = torch.randn(T, k, N, device=DEV, dtype=torch.bfloat16)
    o1, o2 = torch.empty(T, N, device=DEV, dtype=torch.bfloat16), torch.empty(T, N, device=DEV, dtype=torch.bfloat16)
    kernels.moe_sum(y, o1)
    shim.moe_sum_out(y, o2)
    assert torch.equal(o1, o2)
