"""GPU tests of the fp8 (e4m3) grouped GEMM (include/slm_hip.h section 16, slm_moe_fp8_gemm; csrc/moe_gemm_fp8.hip)
and of FusedMoE over fp8 experts.  Three yardsticks: the dense grouped GEMM on the converted weights, bit for bit
(it pins the k order, the fragment halves and the tail units against a kernel that is already pinned); float64 on
the e4m3 values themselves, exactly where the inputs allow it; and the project's GEMM_TOL on random inputs.  Every
run writes into a NaN-filled C followed by a guard row: the guard stays NaN and no output row holds one."""
import numpy as np
import pytest
import torch

from . import moe_fp8_ref as fref
from . import moe_ref as ref
from .moe_fp8_ref import GEMM_TOL, LAUNCH_BLOCKS, as64, rel_err, rounded, torch_dtype

pytestmark = pytest.mark.gpu
DEV = "cuda"
BITS = ["bf16", "f16"]


def _nan_c(n_flat, n_out, dt):
    return torch.full((n_flat + 1, n_out), float("nan"), device=DEV, dtype=dt)


def _run(a, w8, scale, ids, E, a_div, blocks=None, row_scale=None, silu=False, dense=False):
    """one grouped GEMM into a NaN-filled C [n_flat, N_out] followed by a guard row; dense: the f16 / bf16 kernel on
    the converted weights instead"""
    from scalellm_amd import kernels
    n_flat, n_out = ids.size, w8.size(1) // 2 if silu else w8.size(1)
    srt, eid, npad = fref.aligned(ids, E, DEV, blocks)
    full = _nan_c(n_flat, n_out, a.dtype)
    if dense:
        assert scale is None
        kernels.moe_grouped_gemm(a.to(DEV), w8.to(a.dtype).to(DEV), full[:n_flat], srt, eid, npad, a_div,
                                 row_scale=row_scale, silu_mul=silu)
    else:
        kernels.moe_fp8_grouped_gemm(a.to(DEV), w8.to(DEV), None if scale is None else scale.to(DEV), full[:n_flat],
                                     srt, eid, npad, a_div, row_scale=row_scale, silu_mul=silu)
    assert bool(torch.isnan(full[n_flat]).all())                   # the guard row stays NaN
    assert not bool(torch.isnan(full[:n_flat]).any())              # every row of [n_flat] is written
    return full[:n_flat]


def _randn_w8(rng, E, N, K):
    """randn rounded to e4m3: every exponent a unit normal reaches, no scale"""
    return torch.from_numpy(rng.standard_normal((E, N, K)).astype(np.float32)).to(torch.float8_e4m3fn)


def _f32(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(DEV)


# ---- the same bits as the dense kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", LAUNCH_BLOCKS)
@pytest.mark.parametrize("bits", BITS)
def test_same_bits_as_the_dense_kernel_on_the_converted_weights(bits, blocks):
    rng = np.random.default_rng(31)
    for K, N, E, T, k in fref.SAME_BITS_CASES:
        w8 = _randn_w8(rng, E, N, K)
        for a_div in (k, 1):
            a = rounded(rng.standard_normal((T * k // a_div, K)), bits)
            ids = fref.routing(rng, T, k, E, crowd=True)               # expert 0 takes T = 33 rows: two blocks
            what = (K, N, a_div, blocks)
            assert torch.equal(_run(a, w8, None, ids, E, a_div, blocks),
                               _run(a, w8, None, ids, E, a_div, blocks, dense=True)), what
            rs = _f32(rng.random(T * k) + 0.05)
            assert torch.equal(_run(a, w8, None, ids, E, a_div, blocks, row_scale=rs),
                               _run(a, w8, None, ids, E, a_div, blocks, row_scale=rs, dense=True)), (what, "row_scale")
    K, N, E, T, k = fref.SAME_BITS_SILU
    w8 = _randn_w8(rng, E, N, K)
    for a_div in (k, 1):
        a = rounded(rng.standard_normal((T * k // a_div, K)), bits)
        ids = fref.routing(rng, T, k, E, crowd=True)
        assert torch.equal(_run(a, w8, None, ids, E, a_div, blocks, silu=True),
                           _run(a, w8, None, ids, E, a_div, blocks, silu=True, dense=True)), (a_div, blocks, "silu")


# ---- every code converts exactly ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_every_e4m3_code_converts_exactly(bits):
    """A = the 256 unit vectors, so C[t, n] IS the weight W[e(t)][n, t]: 0 ulp against the format's own table"""
    E, N, K = 2, 32, 256
    sweep = fref.code_sweep_weight(N, K)
    w8 = torch.stack([torch.roll(sweep, e, dims=0) for e in range(E)])          # [E, N, K] uint8
    assert np.unique(w8.numpy()).size == 254                                    # every non-NaN code
    a = torch.eye(K, dtype=torch_dtype(bits))
    ids = (np.arange(K, dtype=np.int32) % E).reshape(K, 1)
    out = _run(a, w8, None, ids, E, 1)
    want = fref.e4m3_value(w8.numpy())[ids.reshape(-1), :, np.arange(K)]        # [t, n] = W[e(t)][n, t]
    assert want.shape == (K, N) and np.array_equal(as64(out), want)


# ---- exact: small integers, every element bit for bit -------------------------------------------------------------------
def _int_a(rng, bits, rows, K):
    return rounded(rng.integers(-2, 3, size=(rows, K)), bits)


def _scales(rng, E, N):
    return rng.choice(fref.SCALE_CHOICES, size=(E, N))


@pytest.mark.parametrize("blocks", LAUNCH_BLOCKS)
@pytest.mark.parametrize("bits", BITS)
def test_exact_on_small_integers(bits, blocks):
    """|a| <= 2, integer |w| <= 3 (e4m3 numbers), K = 640: every partial sum is an integer below 2^12, exact in fp32
    in any order; channel scales from {0.25, 0.5, 1, 2} and power-of-two row scales commute with the one rounding.
    The kernel must return the float64 result rounded once."""
    K, N, E, T, k = fref.EXACT_CASE
    rng = np.random.default_rng(5)
    for a_div in (k, 1):
        a, w8 = _int_a(rng, bits, T * k // a_div, K), fref.int_experts(rng, E, N, K)
        scale = _scales(rng, E, N)
        ids = fref.routing(rng, T, k, E, crowd=(a_div == 1))
        want = fref.grouped_fp8_ref(as64(a), w8, scale, ids, a_div)
        out = _run(a, w8, _f32(scale), ids, E, a_div, blocks)
        assert torch.equal(out.cpu(), rounded(want, bits)), (a_div, blocks)
        rs = 2.0 ** rng.integers(-3, 3, size=T * k)
        out = _run(a, w8, _f32(scale), ids, E, a_div, blocks, row_scale=_f32(rs))
        assert torch.equal(out.cpu(), rounded(want * rs[:, None], bits)), (a_div, blocks, "row_scale")


@pytest.mark.parametrize("bits", BITS)
def test_exact_with_a_k_tail(bits):
    """K = 32, 96 (tail units only) and 160, 480 (chunks, then one and three tail units)"""
    N, E, T, k = fref.TAIL_CASE
    rng = np.random.default_rng(6)
    for K in fref.TAIL_KS:
        a, w8 = _int_a(rng, bits, T, K), fref.int_experts(rng, E, N, K)
        scale = _scales(rng, E, N)
        ids = fref.routing(rng, T, k, E, crowd=True)
        want = fref.grouped_fp8_ref(as64(a), w8, scale, ids, k)
        assert torch.equal(_run(a, w8, _f32(scale), ids, E, k).cpu(), rounded(want, bits)), K


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("bits", BITS)
def test_scale_indexing(bits, silu):
    """w_scale[e, n] = 2^((e + n) % 5 - 2) over all-ones weights: a scale taken from another expert or column changes
    whole elements.  Under SiLU * mul the gate and the up column of an output carry different scales."""
    K, N, E, T, k = 160, 320, 8, 33, 2
    rng = np.random.default_rng(7)
    a = _int_a(rng, bits, T, K)
    w8 = fref.to_w8(np.ones((E, N, K)))
    scale = 2.0 ** ((np.arange(E)[:, None] + np.arange(N)[None, :]) % 5 - 2)
    ids = fref.routing(rng, T, k, E, crowd=True)
    want = fref.grouped_fp8_ref(as64(a), w8, scale, ids, k)                      # |sum a| <= 320, times 2^-2 .. 2^2
    assert np.array_equal(want, as64(rounded(want, "bf16")))                    # ... exact in both dtypes
    plain = _run(a, w8, _f32(scale), ids, E, k)
    assert torch.equal(plain.cpu(), rounded(want, bits))
    if silu:
        from scalellm_amd import kernels
        fused = _run(a, w8, _f32(scale), ids, E, k, silu=True)
        unfused = torch.empty_like(fused)
        kernels.silu_and_mul(unfused, plain.contiguous())
        assert torch.equal(fused, unfused)


# ---- random inputs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_project_grid(bits):
    E, k = fref.PROJECT_E, fref.PROJECT_TOPK
    for n, (K, N, T, ad) in enumerate(fref.PROJECT_CASES):
        rng = np.random.default_rng(2000 + n)
        a_div = k if ad == "k" else 1
        a = rounded(rng.standard_normal((T * k // a_div, K)), bits)
        w8, scale = fref.quantized_experts(rng, E, N, K)
        ids = fref.routing(rng, T, k, E, crowd=True)                 # expert 0 takes T rows: T = 33 -> two blocks
        out = _run(a, w8, scale, ids, E, a_div)
        what = (K, N, T, a_div)
        err = rel_err(as64(out), fref.grouped_fp8_ref(as64(a), w8, as64(scale), ids, a_div))
        assert err < GEMM_TOL[bits], (what, err)
        assert torch.equal(_run(a, w8, scale, ids, E, a_div), out), what     # a second run: bit-identical


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("K,N,E,T,k", fref.SILU_CASES)
def test_silu_mul_is_bit_identical_to_the_unfused_sequence(bits, K, N, E, T, k):
    from scalellm_amd import kernels
    rng = np.random.default_rng(K + N + E + T)
    a = rounded(rng.standard_normal((T, K)), bits)
    w8, scale = fref.quantized_experts(rng, E, N, K)
    ids = fref.routing(rng, T, k, E)
    unfused = _run(a, w8, scale, ids, E, k)
    want = torch.empty(T * k, N // 2, device=DEV, dtype=a.dtype)
    kernels.silu_and_mul(want, unfused.contiguous())
    for blocks in (LAUNCH_BLOCKS if N == 320 else (None,)):
        out = _run(a, w8, scale, ids, E, k, blocks, silu=True)
        assert torch.equal(out, want), blocks
    # ... and it is the right function: silu(gate) * up of the fp64 reference; two GEMM outputs meet in one product
    r = fref.grouped_fp8_ref(as64(a), w8, as64(scale), ids, k)
    gate, up = r[:, :N // 2], r[:, N // 2:]
    err = rel_err(as64(out), gate / (1 + np.exp(-gate)) * up)
    assert err < 2 * GEMM_TOL[bits], err


# ---- strides ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_strided_operands(bits):
    """lda > K, ldw = K + 48, an expert stride > N * ldw, w_scale_expert_stride > N, C a column slice of a wider buffer"""
    from scalellm_amd import kernels
    K, N, E, T, k = 160, 96, 8, 33, 2
    rng = np.random.default_rng(8)
    a, w8 = _int_a(rng, bits, T, K), fref.int_experts(rng, E, N, K)
    scale = _scales(rng, E, N)
    ids = fref.routing(rng, T, k, E, crowd=True)
    want = rounded(fref.grouped_fp8_ref(as64(a), w8, scale, ids, k), bits)
    dt = torch_dtype(bits)
    a_wide = torch.full((T, K + 24), float("nan"), device=DEV, dtype=dt)
    a_wide[:, :K] = a.to(DEV)
    w_wide = torch.full((E, N + 3, K + 48), 0x7F, device=DEV, dtype=torch.uint8)      # the padding is the NaN code
    w_wide[:, :N, :K] = w8.view(torch.uint8).to(DEV)
    s_wide = torch.full((E, N + 5), float("nan"), device=DEV)
    s_wide[:, :N] = _f32(scale)
    a_v, w_v, s_v = a_wide[:, :K], w_wide[:, :N, :K], s_wide[:, :N]
    assert a_v.stride(0) > K and w_v.stride(1) == K + 48 and w_v.stride(0) > N * w_v.stride(1) and s_v.stride(0) > N
    c_wide = torch.full((T * k + 1, N + 16), float("nan"), device=DEV, dtype=dt)
    c_v = c_wide[:T * k, 8:8 + N]
    srt, eid, npad = fref.aligned(ids, E, DEV)
    kernels.moe_fp8_grouped_gemm(a_v, w_v, s_v, c_v, srt, eid, npad, k)                # uint8 viewed as e4m3
    assert torch.equal(c_v.cpu(), want)
    keep = torch.ones_like(c_wide, dtype=torch.bool)
    keep[:T * k, 8:8 + N] = False
    assert bool(torch.isnan(c_wide[keep]).all())                     # the other columns and the guard row stay NaN


# ---- dead blocks -------------------------------------------------------------------------------------------------------------
def test_blocks_beyond_n_padded_and_foreign_expert_ids_store_nothing():
    from scalellm_amd import kernels
    K, N, E, T, k = 384, 128, 8, 33, 2
    rng = np.random.default_rng(9)
    a, w8 = _int_a(rng, "bf16", T, K), fref.int_experts(rng, E, N, K)
    scale = _scales(rng, E, N)
    ids = fref.routing(rng, T, k, E, crowd=True)                      # flat index 0 belongs to expert 0
    want = rounded(fref.grouped_fp8_ref(as64(a), w8, scale, ids, k), "bf16")
    a, w8, scale = a.to(DEV), w8.to(DEV), _f32(scale)
    srt, eid, npad = fref.aligned(ids, E, DEV, blocks=40)
    n_live = int(npad[0]) // 32
    assert n_live < 40
    # the tail would overwrite row 0 with expert 3's result if it were computed
    srt[n_live * 32:] = 0
    eid[n_live:] = 3
    out = _nan_c(T * k, N, torch.bfloat16)
    kernels.moe_fp8_grouped_gemm(a, w8, scale, out[:T * k], srt, eid, npad, k)
    assert torch.equal(out[:T * k].cpu(), want) and bool(torch.isnan(out[T * k]).all())
    # an expert id outside [0, E) in a live block: its rows stay untouched, the others are computed
    for foreign in (E, -1):
        eid2 = eid.clone()
        eid2[1] = foreign
        rows = srt[32:64]
        rows = rows[rows < T * k].long()
        out = _nan_c(T * k, N, torch.bfloat16)
        kernels.moe_fp8_grouped_gemm(a, w8, scale, out[:T * k], srt, eid2, npad, k)
        torch.cuda.synchronize()
        assert rows.numel() > 0 and bool(torch.isnan(out[rows]).all())
        mask = torch.ones(T * k, dtype=torch.bool)
        mask[rows.cpu()] = False
        assert torch.equal(out[:T * k].cpu()[mask], want[mask])


# ---- FusedMoE over fp8 experts ---------------------------------------------------------------------------------------------
HID, INTER = fref.MOE_LAYER["hidden"], fref.MOE_LAYER["intermediate"]
NE, TOPK = fref.MOE_LAYER["n_experts"], fref.MOE_LAYER["topk"]


def _moe_layer(bits, scoring, max_tokens=70, seed=0):
    """a Mixtral-FP8 style checkpoint: per-tensor scales, different for w1, w3 and w2 of every expert"""
    from scalellm_amd import kernels, moe
    from scalellm_amd.layers import QuantArgs
    dt = torch_dtype(bits)
    g = torch.Generator().manual_seed(seed)
    sd, values = {}, {}
    for e in range(NE):
        for i, (w, shape) in enumerate((("w1", (INTER, HID)), ("w3", (INTER, HID)), ("w2", (HID, INTER)))):
            w8, s = kernels.quantize_fp8_weight(torch.randn(*shape, generator=g) / (12 + 4 * i), "tensor")
            sd[f"experts.{e}.{w}.weight"], sd[f"experts.{e}.{w}.weight_scale"] = w8, s[0].clone()
            values[f"experts.{e}.{w}"] = (fref.w8_as64(w8), float(s[0]))
        assert values[f"experts.{e}.w1"][1] != values[f"experts.{e}.w3"][1]
    sd["gate.weight"] = (torch.randn(NE, HID, generator=g) * 0.5).to(dt)
    sd["gate.e_score_correction_bias"] = torch.randn(NE, generator=g) * 0.1
    layer = moe.FusedMoE(HID, INTER, NE, TOPK, QuantArgs("fp8", 8), scoring=scoring, renormalize=True,
                         n_expert_groups=4, topk_group=2, scaling_factor=1.5, max_tokens=max_tokens, dtype=dt,
                         device=DEV)
    layer.load_state_dict(sd)
    assert isinstance(layer.experts, moe.MoEFp8Experts)
    return layer, values


def _moe_reference(layer, values, x, bits):
    """the fp64 composition over the e4m3 values and their scales, rounding to the dtype where the layer stores: after
    SiLU * mul (of the rounded gate and up), after the row scale and after the sum"""
    rnd = lambda v: as64(rounded(v, bits))  # noqa: E731
    mm = lambda key, v: (values[key][0] @ v) * values[key][1]  # noqa: E731
    logits = (x.float() @ layer.gate_weight.float().t()).cpu().numpy()
    if layer.scoring == "softmax":
        w, ids = ref.topk_softmax(logits, TOPK, renormalize=True)
    else:
        w, ids = ref.grouped_topk_sigmoid(logits, layer.correction_bias.cpu().numpy(), 4, 2, TOPK, 1.5)
    x64 = as64(x)
    out = np.zeros((x.size(0), HID))
    for t in range(x.size(0)):
        for j in range(TOPK):
            e = int(ids[t, j])
            gate, up = rnd(mm(f"experts.{e}.w1", x64[t])), rnd(mm(f"experts.{e}.w3", x64[t]))
            act = rnd(gate / (1 + np.exp(-gate)) * up)
            out[t] += rnd(np.float32(w[t, j]).astype(np.float64) * mm(f"experts.{e}.w2", act))
    return rnd(out)


@pytest.mark.parametrize("scoring", ["softmax", "grouped_sigmoid"])
@pytest.mark.parametrize("bits", BITS)
def test_fused_moe_fp8_end_to_end(bits, scoring):
    layer, values = _moe_layer(bits, scoring)
    g = torch.Generator(device=DEV).manual_seed(11)
    for T in fref.MOE_TOKENS:
        x = torch.randn(T, HID, device=DEV, dtype=torch_dtype(bits), generator=g)
        y = layer(x)
        want = _moe_reference(layer, values, x, bits)
        assert y.shape == x.shape and not bool(torch.isnan(y).any())
        err = rel_err(as64(y), want)
        assert err < 2 * GEMM_TOL[bits], (T, err)      # two chained GEMMs, GEMM_TOL each
        assert torch.equal(layer(x), y)                # bit-identical repeats
    assert layer.experts.nbytes() == 3 * NE * HID * INTER + 4 * NE * (2 * INTER + HID)


@pytest.mark.parametrize("scoring", ["softmax", "grouped_sigmoid"])
def test_fused_moe_fp8_graph_replay_matches_eager(scoring):
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
    with torch.cuda.graph(graph):                                  # one forward, captured on one stream
        layer.forward(x_static, out=out_static)
    for x, want in zip(xs, eager):
        x_static.copy_(x)
        graph.replay()
        assert torch.equal(out_static, want)
    torch.cuda.synchronize()


# ---- the C++ shim ------------------------------------------------------------------------------------------------------------
def test_shim_fp8_grouped_gemm_matches_the_ctypes_path():
    from scalellm_amd import kernels
    from scalellm_amd.cpp_host import load_shim
    shim = load_shim()
    K, N, E, T, k = 384, 128, 8, 33, 2
    rng = np.random.default_rng(12)
    a = rounded(rng.standard_normal((T, K)), "bf16").to(DEV)
    w8, scale = fref.quantized_experts(rng, E, N, K)
    w8, scale = w8.to(DEV), scale.to(DEV)
    ids = fref.routing(rng, T, k, E)
    srt, eid, npad = fref.aligned(ids, E, DEV)
    rs = torch.rand(T * k, device=DEV) + 0.05
    for silu, row_scale, ws in ((False, None, scale), (False, rs, scale), (True, None, scale), (False, None, None)):
        n_out = N // 2 if silu else N
        c1 = torch.zeros(T * k, n_out, device=DEV, dtype=torch.bfloat16)
        c2 = torch.zeros_like(c1)
        kernels.moe_fp8_grouped_gemm(a, w8, ws, c1, srt, eid, npad, k, row_scale=row_scale, silu_mul=silu)
        shim.moe_fp8_grouped_gemm(a, w8, ws, c2, srt, eid, npad, k, row_scale, silu)
        assert torch.equal(c1, c2) and bool((c1 != 0).any())
