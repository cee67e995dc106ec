"""GPU tests of the dense f16 / bf16 grouped GEMM (include/slm_hip.h section 10, slm_moe_gemm; csrc/moe_gemm.hip)
and of FusedMoE over unquantised experts.  The reference is fp64 numpy over the dtype-rounded inputs, per flat index
A[f // a_div] @ W[e].T (tests/moe_dense_ref.py), as grouped_gemm_ref of the reference's own test does in the kernel's
dtype (src/kernels/gemm/tests/sm80_grouped_gemm_test.cu)."""
import numpy as np
import pytest
import torch

from . import moe_dense_ref as dref
from . import moe_ref as ref
from .moe_dense_ref import GEMM_TOL, as64, rel_err, torch_dtype

pytestmark = pytest.mark.gpu
DEV = "cuda"

# expert_ids.numel() sizes the grid and, with N, decides the columns per workgroup (moe_gemm_waves in moe_gemm.hip:
# the widest of 128 / 64 / 32 columns that still gives 256 workgroups).  At N = 160 (5 tiles of 32 columns; SiLU * mul:
# N = 320, 5 output tiles) None = the capacity rule -> 32 (SiLU: 64) columns, 100 blocks -> 64 (SiLU: 128), 128 -> 128.
# A wave's arithmetic is the same in all of them: the results must be too.
LAUNCH_BLOCKS = (None, 100, 128)


def _inputs(rng, bits, T, K, N, E, k, a_div, scale=1.0):
    a = dref.rounded(rng.standard_normal((T * k // a_div, K)) * scale, bits)
    w = dref.rounded(rng.standard_normal((E, N, K)) * scale, bits)
    return a, w


def _run(a, w, ids, E, a_div, blocks=None, row_scale=None, silu=False):
    """one grouped GEMM into a NaN-filled C [n_flat, N_out] followed by a guard row, which must stay NaN"""
    from scalellm_amd import kernels
    n_flat, n_out = ids.size, w.size(1) // 2 if silu else w.size(1)
    srt, eid, npad = dref.aligned(ids, E, DEV, blocks)
    full = torch.full((n_flat + 1, n_out), float("nan"), device=DEV, dtype=a.dtype)
    kernels.moe_grouped_gemm(a.to(DEV), w.to(DEV), full[:n_flat], srt, eid, npad, a_div, row_scale=row_scale,
                             silu_mul=silu)
    assert bool(torch.isnan(full[n_flat]).all())                   # the guard row stays NaN
    return full[:n_flat]


# ---- the reference's grid ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_reference_grid(bits):
    tol = dref.REF_ALLCLOSE[bits]
    for n, (m, N, K, E, topk) in enumerate(dref.REF_CASES):
        rng = np.random.default_rng(n)
        a, w = _inputs(rng, bits, m, K, N, E, topk, topk, scale=0.1)
        ids = dref.routing(rng, m, topk, E)
        out = _run(a, w, ids, E, topk)
        what = (m, N, K, E, topk)
        o = as64(out)
        assert not np.isnan(o).any(), what                           # every row of [n_flat] is written
        want = dref.grouped_ref(as64(a), as64(w), ids, topk)
        worst = float(np.max(np.abs(o - want) / (tol + tol * np.abs(want))))
        assert dref.allclose(o, want, tol), (what, worst)
        assert torch.equal(_run(a, w, ids, E, topk), out), what      # a second run: bit-identical


# ---- the project's grid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_project_grid(bits):
    E, k = dref.PROJECT_E, dref.PROJECT_TOPK
    for n, (K, N, T, ad) in enumerate(dref.PROJECT_CASES):
        rng = np.random.default_rng(1000 + n)
        a_div = k if ad == "k" else 1
        a, w = _inputs(rng, bits, T, K, N, E, k, a_div)
        ids = dref.routing(rng, T, k, E, crowd=True)                 # expert 0 takes T rows: T = 33 -> two blocks
        out = _run(a, w, ids, E, a_div)
        what = (K, N, T, a_div)
        o = as64(out)
        assert not np.isnan(o).any(), what
        err = rel_err(o, dref.grouped_ref(as64(a), as64(w), ids, a_div))
        assert err < GEMM_TOL[bits], (what, err)
        assert torch.equal(_run(a, w, ids, E, a_div), out), what


# ---- exact: small integers, every element bit for bit ---------------------------------------------------------------
def _int_inputs(rng, bits, T, K, N, E, k, a_div):
    a = dref.rounded(rng.integers(-2, 3, size=(T * k // a_div, K)), bits)
    w = dref.rounded(rng.integers(-3, 4, size=(E, N, K)), bits)
    return a, w


@pytest.mark.parametrize("blocks", LAUNCH_BLOCKS)
@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_exact_on_small_integers(bits, blocks):
    """|a| <= 2, |w| <= 3, K = 640: every partial sum is an integer below 2^12, exact in fp32 in any order, so the
    kernel must return the integer result rounded once to the dtype -- an indexing or k-permutation mistake that a
    tolerance hides changes whole elements here"""
    K, N, E, T, k = 640, 160, 8, 33, 2
    rng = np.random.default_rng(5)
    for a_div in (k, 1):
        a, w = _int_inputs(rng, bits, T, K, N, E, k, a_div)
        ids = dref.routing(rng, T, k, E, crowd=(a_div == 1))
        want = dref.grouped_ref(as64(a), as64(w), ids, a_div)
        assert np.array_equal(want, np.round(want))
        out = _run(a, w, ids, E, a_div, blocks)
        assert torch.equal(out.cpu(), dref.rounded(want, bits)), (a_div, blocks)
        # row scale: powers of two commute with the one rounding
        scale = 2.0 ** rng.integers(-3, 3, size=T * k)
        out = _run(a, w, ids, E, a_div, blocks, row_scale=torch.from_numpy(scale.astype(np.float32)).to(DEV))
        assert torch.equal(out.cpu(), dref.rounded(want * scale[:, None], bits)), (a_div, blocks, "row_scale")


@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_exact_with_a_k_tail(bits):
    """K = 32, 96 (tail units only) and 160, 480 (chunks, then one and three tail units)"""
    rng = np.random.default_rng(6)
    for K in (32, 96, 160, 480):
        a, w = _int_inputs(rng, bits, 33, K, 96, 4, 2, 2)
        ids = dref.routing(rng, 33, 2, 4, crowd=True)
        want = dref.grouped_ref(as64(a), as64(w), ids, 2)
        assert torch.equal(_run(a, w, ids, 4, 2).cpu(), dref.rounded(want, bits)), K


# ---- strides ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_strided_operands(bits):
    """lda > K, ldw > K, ldc > N, an expert stride > N * ldw, C a column slice of a wider buffer"""
    from scalellm_amd import kernels
    K, N, E, T, k = 160, 96, 8, 33, 2
    rng = np.random.default_rng(8)
    a, w = _int_inputs(rng, bits, T, K, N, E, k, k)
    ids = dref.routing(rng, T, k, E, crowd=True)
    want = dref.rounded(dref.grouped_ref(as64(a), as64(w), ids, k), bits)
    dt = torch_dtype(bits)
    a_wide = torch.full((T, K + 24), float("nan"), device=DEV, dtype=dt)
    a_wide[:, :K] = a.to(DEV)
    w_wide = torch.full((E, N + 3, K + 40), float("nan"), device=DEV, dtype=dt)
    w_wide[:, :N, :K] = w.to(DEV)
    a_v, w_v = a_wide[:, :K], w_wide[:, :N, :K]
    assert a_v.stride(0) > K and w_v.stride(1) > K and w_v.stride(0) > N * w_v.stride(1)
    c_wide = torch.full((T * k + 1, N + 16), float("nan"), device=DEV, dtype=dt)
    c_v = c_wide[:T * k, 8:8 + N]
    srt, eid, npad = dref.aligned(ids, E, DEV)
    kernels.moe_grouped_gemm(a_v, w_v, c_v, srt, eid, npad, k)
    assert torch.equal(c_v.cpu(), want)
    keep = torch.ones_like(c_wide, dtype=torch.bool)
    keep[:T * k, 8:8 + N] = False
    assert bool(torch.isnan(c_wide[keep]).all())                     # the other columns and the guard row stay NaN


# ---- dead blocks ------------------------------------------------------------------------------------------------------
def test_blocks_beyond_n_padded_and_foreign_expert_ids_store_nothing():
    from scalellm_amd import kernels
    K, N, E, T, k = 384, 128, 8, 33, 2
    rng = np.random.default_rng(9)
    a, w = _int_inputs(rng, "bf16", T, K, N, E, k, k)
    ids = dref.routing(rng, T, k, E, crowd=True)                      # flat index 0 belongs to expert 0
    want = dref.rounded(dref.grouped_ref(as64(a), as64(w), ids, k), "bf16")
    srt, eid, npad = dref.aligned(ids, E, DEV, blocks=40)
    n_live = int(npad[0]) // 32
    assert n_live < 40
    # the tail would overwrite row 0 with expert 3's result if it were computed
    srt[n_live * 32:] = 0
    eid[n_live:] = 3
    out = torch.full((T * k + 1, N), float("nan"), device=DEV, dtype=torch.bfloat16)
    kernels.moe_grouped_gemm(a.to(DEV), w.to(DEV), out[:T * k], srt, eid, npad, k)
    assert torch.equal(out[:T * k].cpu(), want) and bool(torch.isnan(out[T * k]).all())
    # an expert id outside [0, E) in a live block: its rows stay untouched, the others are computed
    for foreign in (E, -1):
        eid2 = eid.clone()
        eid2[1] = foreign
        rows = srt[32:64]
        rows = rows[rows < T * k].long()
        out = torch.full((T * k + 1, N), float("nan"), device=DEV, dtype=torch.bfloat16)
        kernels.moe_grouped_gemm(a.to(DEV), w.to(DEV), out[:T * k], srt, eid2, npad, k)
        torch.cuda.synchronize()
        assert rows.numel() > 0 and bool(torch.isnan(out[rows]).all())
        mask = torch.ones(T * k, dtype=torch.bool)
        mask[rows.cpu()] = False
        assert torch.equal(out[:T * k].cpu()[mask], want[mask])


# ---- SiLU * mul ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", ["bf16", "f16"])
@pytest.mark.parametrize("K,N,E,T,k", [(128, 64, 1, 3, 1), (384, 128, 8, 33, 2), (640, 320, 8, 96, 4)])
def test_silu_mul_is_bit_identical_to_the_unfused_sequence(bits, K, N, E, T, k):
    from scalellm_amd import kernels
    rng = np.random.default_rng(K + N + E + T)
    a, w = _inputs(rng, bits, T, K, N, E, k, k)
    ids = dref.routing(rng, T, k, E)
    unfused = _run(a, w, ids, E, k)
    want = torch.empty(T * k, N // 2, device=DEV, dtype=a.dtype)
    kernels.silu_and_mul(want, unfused.contiguous())
    for blocks in (LAUNCH_BLOCKS if N == 320 else (None,)):
        out = _run(a, w, ids, E, k, blocks, silu=True)
        assert torch.equal(out, want), blocks
    # ... and it is the right function: silu(gate) * up of the fp64 reference; two GEMM outputs meet in one product
    r = dref.grouped_ref(as64(a), as64(w), ids, k)
    gate, up = r[:, :N // 2], r[:, N // 2:]
    err = rel_err(as64(out), gate / (1 + np.exp(-gate)) * up)
    assert err < 2 * GEMM_TOL[bits], err


# ---- FusedMoE over unquantised experts ------------------------------------------------------------------------------
HID, INTER, NE, TOPK = 256, 384, 8, 2


def _moe_layer(bits, scoring, max_tokens=70, seed=0):
    from scalellm_amd import moe
    dt = torch_dtype(bits)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for e in range(NE):
        sd[f"experts.{e}.w1.weight"] = (torch.randn(INTER, HID, generator=g) / 16).to(dt)
        sd[f"experts.{e}.w3.weight"] = (torch.randn(INTER, HID, generator=g) / 16).to(dt)
        sd[f"experts.{e}.w2.weight"] = (torch.randn(HID, INTER, generator=g) / 16).to(dt)
    sd["gate.weight"] = (torch.randn(NE, HID, generator=g) * 0.5).to(dt)
    sd["gate.e_score_correction_bias"] = torch.randn(NE, generator=g) * 0.1
    layer = moe.FusedMoE(HID, INTER, NE, TOPK, quant_args=None, scoring=scoring, renormalize=True, n_expert_groups=4,
                         topk_group=2, scaling_factor=1.5, max_tokens=max_tokens, dtype=dt, device=DEV)
    layer.load_state_dict(sd)
    return layer, {key: as64(v) for key, v in sd.items() if key.startswith("experts.")}


def _moe_reference(layer, dense, x, bits):
    """the fp64 composition, rounding to the dtype where the layer stores: after SiLU * mul (of the rounded gate and
    up), after the row scale and after the sum"""
    rnd = lambda v: as64(dref.rounded(v, bits))  # noqa: E731
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
            gate = rnd(dense[f"experts.{e}.w1.weight"] @ x64[t])
            up = rnd(dense[f"experts.{e}.w3.weight"] @ x64[t])
            act = rnd(gate / (1 + np.exp(-gate)) * up)
            out[t] += rnd(np.float32(w[t, j]).astype(np.float64) * (dense[f"experts.{e}.w2.weight"] @ act))
    return rnd(out)


@pytest.mark.parametrize("scoring", ["softmax", "grouped_sigmoid"])
@pytest.mark.parametrize("bits", ["bf16", "f16"])
def test_fused_moe_dense_end_to_end(bits, scoring):
    layer, dense = _moe_layer(bits, scoring)
    g = torch.Generator(device=DEV).manual_seed(11)
    for T in (1, 5, 70):
        x = torch.randn(T, HID, device=DEV, dtype=torch_dtype(bits), generator=g)
        y = layer(x)
        want = _moe_reference(layer, dense, x, bits)
        assert y.shape == x.shape and not bool(torch.isnan(y).any())
        err = rel_err(as64(y), want)
        assert err < 2 * GEMM_TOL[bits], (T, err)      # two chained GEMMs, GEMM_TOL each
        assert torch.equal(layer(x), y)                # bit-identical repeats


@pytest.mark.parametrize("scoring", ["softmax", "grouped_sigmoid"])
def test_fused_moe_dense_graph_replay_matches_eager(scoring):
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


# ---- the C++ shim --------------------------------------------------------------------------------------------------------
def test_shim_grouped_gemm_matches_the_ctypes_path():
    from scalellm_amd import kernels
    from scalellm_amd.cpp_host import load_shim
    shim = load_shim()
    K, N, E, T, k = 384, 128, 8, 33, 2
    rng = np.random.default_rng(12)
    a, w = _inputs(rng, "bf16", T, K, N, E, k, k)
    a, w = a.to(DEV), w.to(DEV)
    ids = dref.routing(rng, T, k, E)
    srt, eid, npad = dref.aligned(ids, E, DEV)
    scale = torch.rand(T * k, device=DEV) + 0.05
    for silu, rs in ((False, None), (False, scale), (True, None)):
        n_out = N // 2 if silu else N
        c1 = torch.zeros(T * k, n_out, device=DEV, dtype=torch.bfloat16)
        c2 = torch.zeros_like(c1)
        kernels.moe_grouped_gemm(a, w, c1, srt, eid, npad, k, row_scale=rs, silu_mul=silu)
        shim.moe_grouped_gemm(a, w, c2, srt, eid, npad, k, rs, silu)
        assert torch.equal(c1, c2) and bool((c1 != 0).any())
