"""GPU tests of the MXFP4 grouped GEMM (include/slm_hip.h section 21, slm_moe_mxfp4_gemm; csrc/moe_gemm.hip) and of
FusedMoE over MXFP4 experts.  Nothing here has a tolerance.  Two yardsticks: the dense grouped GEMM on the dequantised
experts, bit for bit (it pins the k order, the nibble order, the block a scale byte belongs to and the tail units
against a kernel that is already pinned), and float64 on the e2m1 * 2^(e - 127) values themselves where the inputs make
one rounding exact.  Every run writes into a NaN-filled C followed by a guard row: the guard stays NaN and no output
row holds one."""
import numpy as np
import pytest
import torch

from . import moe_mxfp4_ref as mx
from .moe_mxfp4_ref import as64, rounded, torch_dtype

pytestmark = pytest.mark.gpu
DEV = "cuda"
BITS = ["bf16", "f16"]


def _nan_c(n_flat, n_out, dt):
    return torch.full((n_flat + 1, n_out), float("nan"), device=DEV, dtype=dt)


def _run(a, w, scale, lists, a_div, row_scale=None, silu=False):
    """one grouped GEMM into a NaN-filled C [n_flat, N_out] followed by a guard row.  w uint8 [E, N, K/2] with `scale`
    uint8 [E, N, K/32]: the MXFP4 kernel; w of A's dtype [E, N, K] with scale None: the dense kernel"""
    from scalellm_amd import kernels
    srt, eid, npad, n_flat = lists
    n_out = w.size(1) // 2 if silu else w.size(1)
    full = _nan_c(n_flat, n_out, a.dtype)
    if scale is None:
        kernels.moe_grouped_gemm(a, w, full[:n_flat], srt, eid, npad, a_div, row_scale=row_scale, silu_mul=silu)
    else:
        kernels.moe_mxfp4_grouped_gemm(a, w, scale, full[:n_flat], srt, eid, npad, a_div, row_scale=row_scale,
                                       silu_mul=silu)
    assert bool(torch.isnan(full[n_flat]).all())                   # the guard row stays NaN
    assert not bool(torch.isnan(full[:n_flat]).any())              # every row of [n_flat] is written
    return full[:n_flat]


def _lists(ids, E, blocks=None):
    return mx.aligned(ids, E, DEV, blocks) + (ids.size,)


def _f32(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(DEV)


# ---- the same bits as the dense kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", mx.SAME_BITS_KS)
@pytest.mark.parametrize("bits", BITS)
def test_same_bits_as_the_dense_kernel_on_the_dequantised_experts(bits, K):
    """every code, scale bytes 118 .. 126 (exact in both dtypes); plain and row_scale at N = 32, 64, 160, SiLU * mul at
    N = 64 and 192, each over the grids that reach NW = 1 / 2 / 4; a_div = k and 1; expert 0 takes all T = 33 tokens, so
    its rows spill into a second block"""
    E, T, k = mx.SAME_BITS_E, mx.SAME_BITS_T, mx.SAME_BITS_TOPK
    rng = np.random.default_rng(31 + K)
    ids = mx.routing(rng, T, k, E, crowd=True)
    rs = _f32(rng.random(T * k) + 0.05)
    acts = {a_div: rounded(rng.standard_normal((T * k // a_div, K)), bits).to(DEV) for a_div in (k, 1)}
    for N, silu_too in [(N, False) for N in mx.SAME_BITS_NS] + [(N, True) for N in mx.SILU_BLOCKS]:
        p, s = mx.random_experts(rng, E, N, K)
        wd = mx.dequantized(p, s, bits).to(DEV)
        p, s = p.to(DEV), s.to(DEV)
        for blocks in (mx.SILU_BLOCKS if silu_too else mx.LAUNCH_BLOCKS)[N]:
            lists = _lists(ids, E, blocks)
            for a_div, a in acts.items():
                what = (K, N, a_div, blocks)
                if silu_too:
                    assert torch.equal(_run(a, p, s, lists, a_div, silu=True),
                                       _run(a, wd, None, lists, a_div, silu=True)), (what, "silu")
                    continue
                assert torch.equal(_run(a, p, s, lists, a_div), _run(a, wd, None, lists, a_div)), what
                assert torch.equal(_run(a, p, s, lists, a_div, row_scale=rs),
                                   _run(a, wd, None, lists, a_div, row_scale=rs)), (what, "row_scale")


# ---- which nibble -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_every_k_of_a_chunk_and_a_tail_unit_reads_its_own_nibble(bits):
    """K = 160: one chunk and one tail unit.  A = the 160 unit vectors (a_div = 1: flat index f reads row f), the code
    of W[e][n, k] is (e + n + k) mod 16 under block scales that differ along the row: C[f, n] IS the weight
    W[e(f)][n, f], 0 ulp against the format's own table.  A swapped nibble pair, a shifted dword or a neighbour's
    scale changes every element of a row."""
    E, N, K = 2, 32, 160
    p, s = mx.code_sweep_experts(E, N, K)
    assert np.unique(mx.mref.unpack(p[0])).size == 16
    ids = ((np.arange(K // 2)[:, None] + np.arange(2)[None, :]) % E).astype(np.int32)   # [T = 80, k = 2]
    a = torch.eye(K, dtype=torch_dtype(bits), device=DEV)
    out = _run(a, p.to(DEV), s.to(DEV), _lists(ids, E), 1)
    want = mx.experts_as64(p, s)[ids.reshape(-1), :, np.arange(K)]                       # [f, n] = W[e(f)][n, f]
    assert want.shape == (K, N) and np.count_nonzero(want) > K * N // 2
    assert np.array_equal(as64(out), want)


# ---- which scale byte ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [160, 96], ids=["chunk+tail", "tail3"])
@pytest.mark.parametrize("bits", BITS)
def test_every_block_takes_its_own_scale_byte(bits, K):
    """all codes 1.0, the scale byte of block (e, n, b) from moe_mxfp4_ref.scale_pattern (neighbours in e, n and b never
    share one), A one-hot at one k per block: C == 2^(byte - 127) exactly for every (e, n, block) -- the last block of
    the tail and the last expert included.  Then the same through a padded row stride, a padded expert stride and a
    base one byte off any alignment, the padding holding 0xFF (the MX NaN)."""
    from scalellm_amd import kernels
    E, N, nb = 4, 64, K // 32
    s = mx.scale_pattern(E, N, nb, bits)
    p = torch.full((E, N, K // 2), 0x22, dtype=torch.uint8)
    T = E * nb                                                     # token t: expert t % E, block t // E; k = 1
    ids = (np.arange(T, dtype=np.int32) % E).reshape(T, 1)
    a = torch.zeros(T, K, dtype=torch_dtype(bits))
    for t in range(T):
        b = t // E
        a[t, 32 * b + (7 * b + 3 * (t % E) + 5) % 32] = 1.0
    want = np.exp2(s.numpy().astype(np.float64) - 127)[np.arange(T) % E, :, np.arange(T) // E]    # [t, n]
    assert want.shape == (T, N) and np.array_equal(as64(rounded(want, bits)), want)
    lists = _lists(ids, E)
    a, p = a.to(DEV), p.to(DEV)
    out = _run(a, p, s.to(DEV), lists, 1)
    assert np.array_equal(as64(out), want)
    # lds = nb + 3, expert stride = N * lds + 7, base offset 1: nothing about the scales is aligned
    lds, es = nb + 3, N * (nb + 3) + 7
    buf = torch.full((1 + E * es + 16,), 0xFF, dtype=torch.uint8, device=DEV)
    s_v = buf.as_strided((E, N, nb), (es, lds, 1), 1)
    s_v.copy_(s.to(DEV))
    assert s_v.data_ptr() % 2 == 1 and s_v.stride(1) == lds and s_v.stride(0) == es
    out = _run(a, p, s_v, lists, 1)
    assert np.array_equal(as64(out), want)
    assert int((buf == 0xFF).sum()) == buf.numel() - E * N * nb    # the test wrote the pattern only where it belongs
    # ... and a lone expert (E = 1: its stride is made up by the wrapper) at the odd base
    one = _lists(np.zeros((nb, 1), np.int32), 1)
    a1 = a[::E].contiguous()                                       # tokens 0, E, 2 E, ...: blocks 0 .. nb - 1
    full = _nan_c(nb, N, a.dtype)
    kernels.moe_mxfp4_grouped_gemm(a1, p[:1], s_v[:1], full[:nb], one[0], one[1], one[2], 1)
    assert np.array_equal(as64(full[:nb]), np.exp2(s[0].numpy().astype(np.float64) - 127).T)


# ---- exact: small integers, every element bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("K", [672, 96])
@pytest.mark.parametrize("bits", BITS)
def test_exact_on_small_integers(bits, K):
    """mxfp4_ref.int_inputs per expert: every partial sum is a multiple of 1/4 below 2^16, exact in fp32 in any order,
    so the kernel must return the float64 result rounded once; power-of-two row scales commute with that rounding"""
    N, E, T, k = 160, 8, 33, 2
    rng = np.random.default_rng(5 + K)
    a64, p, s = mx.int_experts(rng, E, T, K, N)
    a = rounded(a64, bits)
    for a_div, blocks in ((k, None), (k, 128)):
        ids = mx.routing(rng, T, k, E, crowd=True)
        want = mx.grouped_mxfp4_ref(a64, p, s, ids, a_div)
        lists = _lists(ids, E, blocks)
        out = _run(a.to(DEV), p.to(DEV), s.to(DEV), lists, a_div)
        assert torch.equal(out.cpu(), rounded(want, bits)), (a_div, blocks)
        rsc = 2.0 ** rng.integers(-3, 3, size=T * k)
        out = _run(a.to(DEV), p.to(DEV), s.to(DEV), lists, a_div, row_scale=_f32(rsc))
        assert torch.equal(out.cpu(), rounded(want * rsc[:, None], bits)), (a_div, blocks, "row_scale")


# ---- strides ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_strided_operands_with_poisoned_padding(bits):
    """lda > K, ldw = K/2 + 48, an expert stride > N * ldw, padded scale strides, C a column slice of a wider buffer.
    Every padding byte of W and of the scales is 0xFF (the codes -6 | -6; the MX NaN scale), A's padding NaN: a read
    outside an expert's own rows poisons the result"""
    from scalellm_amd import kernels
    K, N, E, T, k = 416, 96, 8, 33, 2
    rng = np.random.default_rng(8)
    a64, p, s = mx.int_experts(rng, E, T, K, N)
    ids = mx.routing(rng, T, k, E, crowd=True)
    want = rounded(mx.grouped_mxfp4_ref(a64, p, s, ids, k), bits)
    dt = torch_dtype(bits)
    a_wide = torch.full((T, K + 24), float("nan"), device=DEV, dtype=dt)
    a_wide[:, :K] = rounded(a64, bits).to(DEV)
    w_wide = torch.full((E, N + 3, K // 2 + 48), 0xFF, device=DEV, dtype=torch.uint8)
    w_wide[:, :N, :K // 2] = p.to(DEV)
    s_wide = torch.full((E, N + 5, K // 32 + 6), 0xFF, device=DEV, dtype=torch.uint8)
    s_wide[:, :N, :K // 32] = s.to(DEV)
    a_v, w_v, s_v = a_wide[:, :K], w_wide[:, :N, :K // 2], s_wide[:, :N, :K // 32]
    assert a_v.stride(0) > K and w_v.stride(1) == K // 2 + 48 and w_v.stride(0) > N * w_v.stride(1)
    assert s_v.stride(1) == K // 32 + 6 and s_v.stride(0) > N * s_v.stride(1)
    c_wide = torch.full((T * k + 1, N + 16), float("nan"), device=DEV, dtype=dt)
    c_v = c_wide[:T * k, 8:8 + N]
    srt, eid, npad = mx.aligned(ids, E, DEV)
    kernels.moe_mxfp4_grouped_gemm(a_v, w_v, s_v, c_v, srt, eid, npad, k)
    assert torch.equal(c_v.cpu(), want)
    keep = torch.ones_like(c_wide, dtype=torch.bool)
    keep[:T * k, 8:8 + N] = False
    assert bool(torch.isnan(c_wide[keep]).all())                     # the other columns and the guard row stay NaN
    # the [E, N, K/32, 16] blocks view of the same memory (gpt-oss `*_blocks`) is the same call
    w_blk = w_wide.as_strided((E, N, K // 32, 16), (w_wide.stride(0), w_wide.stride(1), 16, 1))
    c2 = torch.full((T * k, N), float("nan"), device=DEV, dtype=dt)
    kernels.moe_mxfp4_grouped_gemm(a_v, w_blk, s_v, c2, srt, eid, npad, k)
    assert torch.equal(c2.cpu(), want)


# ---- dead blocks -------------------------------------------------------------------------------------------------------------
def test_blocks_beyond_n_padded_and_foreign_expert_ids_store_nothing():
    from scalellm_amd import kernels
    K, N, E, T, k = 416, 128, 8, 33, 2
    rng = np.random.default_rng(9)
    a64, p, s = mx.int_experts(rng, E, T, K, N)
    ids = mx.routing(rng, T, k, E, crowd=True)                        # flat index 0 belongs to expert 0
    want = rounded(mx.grouped_mxfp4_ref(a64, p, s, ids, k), "bf16")
    a, p, s = rounded(a64, "bf16").to(DEV), p.to(DEV), s.to(DEV)
    srt, eid, npad = mx.aligned(ids, E, DEV, blocks=40)
    n_live = int(npad[0]) // 32
    assert n_live < 40 and bool((srt[:n_live * 32] >= T * k).any())   # live blocks hold padding indices >= n_flat
    # the tail would overwrite row 0 with expert 3's result if it were computed
    srt[n_live * 32:] = 0
    eid[n_live:] = 3
    out = _nan_c(T * k, N, torch.bfloat16)
    kernels.moe_mxfp4_grouped_gemm(a, p, s, out[:T * k], srt, eid, npad, k)
    assert torch.equal(out[:T * k].cpu(), want) and bool(torch.isnan(out[T * k]).all())
    # an expert id outside [0, E) in a live block: its rows stay untouched, the others are computed
    for foreign in (E, -1):
        eid2 = eid.clone()
        eid2[1] = foreign
        rows = srt[32:64]
        rows = rows[rows < T * k].long()
        out = _nan_c(T * k, N, torch.bfloat16)
        kernels.moe_mxfp4_grouped_gemm(a, p, s, out[:T * k], srt, eid2, npad, k)
        torch.cuda.synchronize()
        assert rows.numel() > 0 and bool(torch.isnan(out[rows]).all())
        mask = torch.ones(T * k, dtype=torch.bool)
        mask[rows.cpu()] = False
        assert torch.equal(out[:T * k].cpu()[mask], want[mask])


# ---- FusedMoE over MXFP4 experts -------------------------------------------------------------------------------------------
HID, INTER = mx.MOE_LAYER["hidden"], mx.MOE_LAYER["intermediate"]
NE, TOPK = mx.MOE_LAYER["n_experts"], mx.MOE_LAYER["topk"]


def _moe_layers(bits, scoring, max_tokens=70, seed=0):
    """(FusedMoE over the MXFP4 checkpoint, FusedMoE(quant_args=None) over the same checkpoint dequantised): the same
    router weights, so the same routing"""
    from scalellm_amd import moe
    from scalellm_amd.layers import QuantArgs
    dt = torch_dtype(bits)
    sd = mx.mxfp4_state_dict(HID, INTER, NE, bits, seed)
    kw = dict(scoring=scoring, renormalize=True, n_expert_groups=4, topk_group=2, scaling_factor=1.5,
              max_tokens=max_tokens, dtype=dt, device=DEV)
    q = moe.FusedMoE(HID, INTER, NE, TOPK, QuantArgs("mxfp4", 4), **kw)
    q.load_state_dict(sd)
    d = moe.FusedMoE(HID, INTER, NE, TOPK, None, **kw)
    d.load_state_dict(mx.dequantized_state_dict(sd, bits))
    assert isinstance(q.experts, moe.MoEMxfp4Experts) and isinstance(d.experts, moe.MoEDenseExperts)
    return q, d


@pytest.mark.parametrize("scoring", ["softmax", "grouped_sigmoid"])
@pytest.mark.parametrize("bits", BITS)
def test_fused_moe_mxfp4_equals_the_dense_layer_on_the_dequantised_experts(bits, scoring):
    q, d = _moe_layers(bits, scoring)
    g = torch.Generator(device=DEV).manual_seed(11)
    for T in mx.MOE_TOKENS:
        x = torch.randn(T, HID, device=DEV, dtype=torch_dtype(bits), generator=g)
        y = q(x)
        assert y.shape == x.shape and bool(torch.isfinite(y).all()) and bool((y != 0).any())
        assert torch.equal(y, d(x)), T
        assert torch.equal(q._buf["ids"][:T * TOPK], d._buf["ids"][:T * TOPK])      # the same routing
        assert torch.equal(q(x), y)                                                # bit-identical repeats
    assert q.experts.gate_up.dtype == torch.uint8
    assert q.experts.nbytes() == 3 * NE * HID * INTER // 2 + 3 * NE * HID * INTER // 32
    assert 3.7 * q.experts.nbytes() < d.experts.nbytes()


@pytest.mark.parametrize("scoring", ["softmax", "grouped_sigmoid"])
def test_fused_moe_mxfp4_graph_replay_matches_eager(scoring):
    T = 5
    layer, _ = _moe_layers("bf16", scoring, max_tokens=T)
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
def test_shim_mxfp4_grouped_gemm_matches_the_ctypes_path():
    from scalellm_amd import kernels
    from scalellm_amd.cpp_host import load_shim
    shim = load_shim()
    K, N, E, T, k = 416, 128, 8, 33, 2
    rng = np.random.default_rng(12)
    a = rounded(rng.standard_normal((T, K)), "bf16").to(DEV)
    p, s = mx.random_experts(rng, E, N, K)
    p, s = p.to(DEV), s.to(DEV)
    ids = mx.routing(rng, T, k, E)
    srt, eid, npad = mx.aligned(ids, E, DEV)
    rs = torch.rand(T * k, device=DEV) + 0.05
    for silu, row_scale in ((False, None), (False, rs), (True, None)):
        n_out = N // 2 if silu else N
        c1 = torch.zeros(T * k, n_out, device=DEV, dtype=torch.bfloat16)
        c2 = torch.zeros_like(c1)
        kernels.moe_mxfp4_grouped_gemm(a, p, s, c1, srt, eid, npad, k, row_scale=row_scale, silu_mul=silu)
        shim.moe_mxfp4_grouped_gemm(a, p, s, c2, srt, eid, npad, k, row_scale, silu)
        assert torch.equal(c1, c2) and bool((c1 != 0).any())
