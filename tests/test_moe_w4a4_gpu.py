"""GPU tests of the grouped W4A4 GEMM (slm_hip.h section 23, csrc/w4a4_moe.hip) and FusedMoE(act_quant="mxfp4"): bit for
bit but for the one random-data case.  T outputs go into a NaN-filled C, byte outputs into 0xFF, plus a guard row."""
import numpy as np
import pytest
import torch

from . import moe_mxfp4_ref as mx
from . import w4a4_ref as wr
from .moe_mxfp4_ref import as64, rounded, torch_dtype

pytestmark = pytest.mark.gpu
DEV = "cuda"
BITS = ["bf16", "f16"]
E, T, TOPK = 3, 33, 2


def _lists(ids, n_experts, blocks=None):
    return mx.aligned(ids, n_experts, DEV, blocks) + (ids.size,)


def _run(a, w, lists, a_div, bits, row_scale=None, silu=False, quant=False, complete=True):
    """a = (codes, scales), w = (codes [E, N, K/2], scales): one launch into poisoned outputs with a guard row"""
    from scalellm_amd import kernels
    srt, eid, npad, n_flat = lists
    N = w[0].size(1)
    if quant:
        cq = torch.full((n_flat + 1, N // 4), 0xFF, dtype=torch.uint8, device=DEV)
        cs = torch.full((n_flat + 1, N // 64), 0xFF, dtype=torch.uint8, device=DEV)
        kernels.moe_w4a4_grouped_gemm(*a, *w, cq[:n_flat], srt, eid, npad, a_div, silu_mul=True, c_scale=cs[:n_flat],
                                      dtype=torch_dtype(bits))
        assert bool((cq[n_flat] == 0xFF).all()) and bool((cs[n_flat] == 0xFF).all())
        return cq[:n_flat], cs[:n_flat]
    full = torch.full((n_flat + 1, N // 2 if silu else N), float("nan"), device=DEV, dtype=torch_dtype(bits))
    kernels.moe_w4a4_grouped_gemm(*a, *w, full[:n_flat], srt, eid, npad, a_div, row_scale=row_scale, silu_mul=silu)
    assert bool(torch.isnan(full[n_flat]).all())
    assert not complete or not bool(torch.isnan(full[:n_flat]).any())
    return full[:n_flat]


def _padded(codes, scale):
    """the same values through padded row strides and a scale base one byte off any alignment, 0xFF in the padding"""
    lead, kb, nb = codes.shape[:-1], codes.shape[-1], scale.shape[-1]
    cp = torch.full(lead + (kb + 16,), 0xFF, dtype=torch.uint8, device=DEV)
    cp[..., :kb] = codes.to(DEV)
    sp = torch.full((1 + int(np.prod(lead)) * (nb + 3),), 0xFF, dtype=torch.uint8, device=DEV)
    sv = sp[1:].view(lead + (nb + 3,))[..., :nb]
    sv.copy_(scale.to(DEV))
    return cp[..., :kb], sv


def _random(rng, rows, K, lo=118, hi=126):
    return (torch.from_numpy(rng.integers(0, 256, size=rows + (K // 2,), dtype=np.uint8)),
            torch.from_numpy(rng.integers(lo, hi + 1, size=rows + (K // 32,)).astype(np.uint8)))


_dev = lambda pair: tuple(t.to(DEV) for t in pair)  # noqa: E731


@pytest.mark.parametrize("K", [32, 96, 128, 160, 416, 672])
@pytest.mark.parametrize("bits", BITS)
def test_integer_inputs_equal_one_rounding_of_float64(bits, K):
    """int_inputs per expert, row_scale powers of two, grids for NW = 1 / 2 / 4, a_div = k and 1, a crowded expert"""
    rng = np.random.default_rng(7 + K)
    ids = mx.routing(rng, T, TOPK, E, crowd=True)
    rs = np.exp2(rng.integers(-2, 2, size=T * TOPK)).astype(np.float32)
    for N in mx.SAME_BITS_NS:
        draws = [wr.int_inputs(rng, T * TOPK, K, N, False) for _ in range(E)]
        aq, asc = draws[0][:2]
        wq, ws = torch.stack([d[2] for d in draws]), torch.stack([d[3] for d in draws])
        w = _padded(wq, ws)
        for a_div in (TOPK, 1):
            rows = T * TOPK // a_div
            want = mx.dref.grouped_ref(wr.w_as64(aq[:rows], asc[:rows]), mx.experts_as64(wq, ws), ids, a_div)
            a = _padded(aq[:rows], asc[:rows])
            for blocks in mx.LAUNCH_BLOCKS[N]:
                lists = _lists(ids, E, blocks)
                assert torch.equal(_run(a, w, lists, a_div, bits).cpu(), rounded(want, bits)), (N, a_div, blocks)
                got = _run(a, w, lists, a_div, bits, row_scale=torch.from_numpy(rs).to(DEV))
                assert torch.equal(got.cpu(), rounded(want * rs[:, None], bits)), (N, a_div, blocks, "row_scale")


@pytest.mark.parametrize("K", [160, 672])
@pytest.mark.parametrize("bits", BITS)
def test_an_experts_rows_are_the_linears_bits_for_every_launch_shape(bits, K):
    """per expert kernels.w4a4_linear (pre-quantised, SLM_W4A4_SPLITK = 1) on its rows; SiLU: then silu_and_mul"""
    from scalellm_amd import kernels
    rng = np.random.default_rng(11 + K)
    ids = mx.routing(rng, T, TOPK, E, crowd=True)
    flat = ids.reshape(-1)
    a = _dev(_random(rng, (T * TOPK,), K))
    for N, silu in [(N, False) for N in mx.SAME_BITS_NS] + [(N, True) for N in mx.SILU_BLOCKS]:
        w = _dev(_random(rng, (E, N), K))
        for a_div in (TOPK, 1):
            rows = T * TOPK // a_div
            want = torch.empty(T * TOPK, N // 2 if silu else N, dtype=torch_dtype(bits), device=DEV)
            with kernels.tuning(SLM_W4A4_SPLITK=1):
                for e in range(E):
                    sel = torch.from_numpy(np.nonzero(flat == e)[0]).to(DEV)
                    src = sel // a_div
                    c = torch.empty(sel.numel(), N, dtype=want.dtype, device=DEV)
                    kernels.w4a4_linear(a[0][src].contiguous(), w[0][e], w[1][e], c, a_scale=a[1][src].contiguous())
                    if silu:
                        act = torch.empty(sel.numel(), N // 2, dtype=want.dtype, device=DEV)
                        kernels.silu_and_mul(act, c)
                        c = act
                    want[sel] = c
            for blocks in (mx.SILU_BLOCKS if silu else mx.LAUNCH_BLOCKS)[N]:
                got = _run((a[0][:rows], a[1][:rows]), w, _lists(ids, E, blocks), a_div, bits, silu=silu)
                assert torch.equal(got, want), (N, silu, a_div, blocks)


@pytest.mark.parametrize("K", [160, 672])
@pytest.mark.parametrize("N", [64, 192])
@pytest.mark.parametrize("bits", BITS)
def test_quantised_output_is_the_quantiser_on_the_silu_output(bits, N, K):
    """scale bytes over 15 binades; N = 192: zero gate codes make output tile 0 all zero (byte 127, -0 codes)"""
    from scalellm_amd import kernels
    rng = np.random.default_rng(13 + N + K)
    ids = mx.routing(rng, T, TOPK, E, crowd=True)
    a = _dev(_random(rng, (T,), K))
    wq, ws = _random(rng, (E, N), K, 115, 129)
    if N == 192:
        wq[:, :32] = 0
    w = _dev((wq, ws))
    for blocks in mx.SILU_BLOCKS[N]:
        lists = _lists(ids, E, blocks)
        act = _run(a, w, lists, TOPK, bits, silu=True)
        want_q, want_s = kernels.quantize_mxfp4_act(act)
        cq, cs = _run(a, w, lists, TOPK, bits, quant=True)
        assert torch.equal(cs, want_s) and torch.equal(cq, want_q), blocks
        assert cs[:, -1].unique().numel() > 3                      # several binades
        assert N == 64 or (bool((cs[:, 0] == 127).all()) and bool((cq[:, :16] == 0x88).any()))


@pytest.mark.parametrize("K", [96, 160], ids=["tail3", "chunk+tail"])
@pytest.mark.parametrize("bits", BITS)
def test_every_block_takes_its_own_scale_bytes_and_its_gathered_row(bits, K):
    """token t: expert t % E, one-hot in block t // E; weights all 1.0: C[t, n] = 2^(as[t, b] + ws[e, n, b] - 254)"""
    n_exp, N, nb = 4, 64, K // 32
    n_tok = n_exp * nb
    ws = mx.scale_pattern(n_exp, N, nb, bits)
    codes = np.zeros((n_tok, K), dtype=np.int64)
    t = np.arange(n_tok)
    codes[t, 32 * (t // n_exp) + (7 * (t // n_exp) + 3 * (t % n_exp) + 5) % 32] = 2
    asc = (121 + (t[:, None] + 3 * np.arange(nb)[None, :]) % 7).astype(np.uint8)
    want = np.exp2(asc[t, t // n_exp].astype(np.float64) - 127)[:, None] * \
        np.exp2(ws.numpy().astype(np.float64) - 127)[t % n_exp, :, t // n_exp]
    assert np.array_equal(as64(rounded(want, bits)), want)
    ids = (t % n_exp).astype(np.int32).reshape(n_tok, 1)
    a = _padded(wr.pack(codes), torch.from_numpy(asc))
    w = _padded(torch.full((n_exp, N, K // 2), 0x22, dtype=torch.uint8), ws)
    assert np.array_equal(as64(_run(a, w, _lists(ids, n_exp), 1, bits)), want)


def test_dead_blocks_and_expert_ids_outside_the_range_leave_their_rows_untouched():
    rng = np.random.default_rng(5)
    K, N = 160, 64
    ids = mx.routing(rng, T, TOPK, E, crowd=True)
    a, w = _dev(_random(rng, (T,), K)), _dev(_random(rng, (E, N), K))
    srt, eid, npad, n_flat = _lists(ids, E)
    want = _run(a, w, (srt, eid, npad, n_flat), TOPK, "bf16")
    n_blocks = int(npad.item()) // 32
    assert n_blocks >= 4
    eid2 = eid.clone()
    eid2[0], eid2[1] = E, -1                                       # outside [0, E)
    npad2 = npad - 32                                              # the last block is dead
    got = _run(a, w, (srt, eid2, npad2, n_flat), TOPK, "bf16", complete=False)
    rows = srt.view(-1, 32).cpu().numpy()
    dead = np.concatenate([rows[0], rows[1], rows[n_blocks - 1]])
    dead = dead[dead < n_flat]
    live = np.setdiff1d(np.arange(n_flat), dead)
    assert dead.size > 32 and bool(torch.isnan(got[dead]).all()) and torch.equal(got[live], want[live])


def test_random_data_against_float64():
    rng = np.random.default_rng(3)
    K, N, n_tok = 672, 160, 70
    ids = mx.routing(rng, n_tok, TOPK, 8)
    a, w = _random(rng, (n_tok,), K), _random(rng, (8, N), K)
    want = mx.dref.grouped_ref(wr.w_as64(*a), mx.experts_as64(*w), ids, TOPK)
    got = as64(_run(_dev(a), _dev(w), _lists(ids, 8), TOPK, "bf16"))
    err = wr.rel_err(got, want)
    print(f"relative error {err:.3e} (bound {wr.GEMM_TOL['bf16']:.1e})")
    assert err <= wr.GEMM_TOL["bf16"]


@pytest.mark.parametrize("bits", BITS)
def test_fused_moe_with_mxfp4_activations_is_its_kernel_sequence_and_replays(bits):
    from scalellm_amd import kernels, moe
    from scalellm_amd.layers import QuantArgs
    dt, cfg = torch_dtype(bits), mx.MOE_LAYER
    H, I, n_exp, k = cfg["hidden"], cfg["intermediate"], cfg["n_experts"], cfg["topk"]
    with pytest.raises(kernels.SlmError, match="mxfp4"):
        moe.FusedMoE(H, I, n_exp, k, QuantArgs("fp8", 8), dtype=dt, device=DEV, act_quant="mxfp4")
    with pytest.raises(kernels.SlmError, match="mxfp4"):
        moe.FusedMoE(H, I, n_exp, k, None, dtype=dt, device=DEV, act_quant="mxfp4")
    layer = moe.FusedMoE(H, I, n_exp, k, QuantArgs("mxfp4", 4), dtype=dt, device=DEV, max_tokens=70, router="fused",
                         act_quant="mxfp4")
    layer.load_state_dict(mx.mxfp4_state_dict(H, I, n_exp, bits))
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(70, H, generator=g).to(dt).to(DEV) for _ in range(3)]
    ex = layer.experts

    def written_out(x):
        n_tok = x.size(0)
        wts, ids = kernels.moe_router(x, layer.gate_weight, k, scoring="softmax", renormalize=True)
        max_padded, max_blocks = kernels.moe_align_capacity(n_tok * k, n_exp, 32)
        srt = torch.empty(max_padded, dtype=torch.int32, device=DEV)
        eid = torch.empty(max_blocks, dtype=torch.int32, device=DEV)
        npad = torch.zeros(1, dtype=torch.int32, device=DEV)
        kernels.moe_align_block(ids, n_exp, 32, srt, eid, npad)
        xq, xsc = kernels.quantize_mxfp4_act(x)
        actq = torch.empty(n_tok * k, I // 2, dtype=torch.uint8, device=DEV)
        acts = torch.empty(n_tok * k, I // 32, dtype=torch.uint8, device=DEV)
        kernels.moe_w4a4_grouped_gemm(xq, xsc, ex.gate_up, ex.gate_up_scale, actq, srt, eid, npad, k, silu_mul=True,
                                      c_scale=acts, dtype=dt)
        down = torch.empty(n_tok * k, H, dtype=dt, device=DEV)
        kernels.moe_w4a4_grouped_gemm(actq, acts, ex.down, ex.down_scale, down, srt, eid, npad, 1,
                                      row_scale=wts.view(-1))
        out = torch.empty(n_tok, H, dtype=dt, device=DEV)
        kernels.moe_sum(down.view(n_tok, k, H), out)
        return out

    for n_tok in mx.MOE_TOKENS:
        got = layer(xs[0][:n_tok])
        assert bool(torch.isfinite(got.float()).all()) and float(got.float().abs().max()) > 0
        assert torch.equal(got, written_out(xs[0][:n_tok])), n_tok
    x, out = xs[0].clone(), torch.empty_like(xs[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer(x, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer(x, out=out)
    for xi in xs:                                                  # the routing changes under the graph
        x.copy_(xi)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, layer(xi)) and torch.equal(out, written_out(xi))
