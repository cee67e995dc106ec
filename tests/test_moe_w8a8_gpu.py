"""GPU tests of the grouped W8A8 GEMM (slm_hip.h section 26) and FusedMoE(act_quant="fp8"): bit for bit but for one
random-data case.  Outputs go into a NaN-filled C with a guard row; padded strides hold 0xFF (NaN in e4m3) or NaN."""
import numpy as np
import pytest
import torch

from . import moe_fp8_ref as fref
from . import moe_mxfp4_ref as mx
from . import w8a8_ref as wr
from .moe_fp8_ref import as64, rounded, torch_dtype

pytestmark = pytest.mark.gpu
DEV, BITS = "cuda", ["bf16", "f16"]
E, T, TOPK = 3, 33, 2


def _lists(ids, n_experts, blocks=None):
    return mx.aligned(ids, n_experts, DEV, blocks) + (ids.size,)


def _run(a, w, lists, a_div, bits, row_scale=None, silu=False, complete=True):
    """a = (aq, a_scale), w = (w8 [E, N, K], w_scale [E, N]): one launch into a NaN-filled C with a guard row"""
    from scalellm_amd import kernels
    srt, eid, npad, n_flat = lists
    N = w[0].size(1)
    full = torch.full((n_flat + 1, N // 2 if silu else N), float("nan"), device=DEV, dtype=torch_dtype(bits))
    kernels.moe_w8a8_grouped_gemm(*a, *w, full[:n_flat], srt, eid, npad, a_div, row_scale=row_scale, silu_mul=silu)
    assert bool(torch.isnan(full[n_flat]).all()) and not (complete and bool(torch.isnan(full[:n_flat]).any()))
    return full[:n_flat]


def _padded(t8, scale):
    """the same values through padded strides: 0xFF behind every row and every expert, NaN behind an expert's scales"""
    rows, K = t8.shape[-2:]
    p = torch.full(tuple(t8.shape[:-2]) + (rows + 1, K + 16), 0xFF, dtype=torch.uint8, device=DEV)
    p[..., :rows, :K] = t8.view(torch.uint8).to(DEV)
    if scale.dim() == 1:
        return p[:rows, :K], scale.to(DEV)
    sp = torch.full((scale.size(0), rows + 4), float("nan"), device=DEV)
    sp[:, :rows] = scale.to(DEV)
    return p[:, :rows, :K], sp[:, :rows]


def _random(rng, rows, K, lo, hi):
    """random e4m3 bytes without the NaN codes, random fp32 scales in [2^lo, 2^hi)"""
    b = rng.integers(0, 256, size=rows + (K,), dtype=np.uint8)
    b[(b & 0x7F) == 0x7F] = 0
    s = np.exp2(rng.uniform(lo, hi, size=rows)).astype(np.float32)
    return torch.from_numpy(b).to(DEV), torch.from_numpy(s).to(DEV)


def _linear_bits(a, w, ids, N, a_div, silu, bits):
    """per expert kernels.w8a8_linear (SLM_W8A8_SPLITK = 1) on its gathered rows; SiLU: then silu_and_mul"""
    from scalellm_amd import kernels
    flat = ids.reshape(-1)
    want = torch.empty(flat.size, N, dtype=torch_dtype(bits), device=DEV)
    with kernels.tuning(SLM_W8A8_SPLITK=1):
        for e in range(w[0].size(0)):
            sel = torch.from_numpy(np.nonzero(flat == e)[0]).to(DEV)
            c = torch.empty(sel.numel(), N, dtype=want.dtype, device=DEV)
            kernels.w8a8_linear(a[0][sel // a_div].contiguous(), a[1][sel // a_div].contiguous(), w[0][e], w[1][e], c)
            want[sel] = c
    if not silu:
        return want
    act = torch.empty(flat.size, N // 2, dtype=want.dtype, device=DEV)
    kernels.silu_and_mul(act, want)
    return act


@pytest.mark.parametrize("K", [32, 96, 128, 160, 416, 672])
@pytest.mark.parametrize("bits", BITS)
def test_integer_inputs_equal_one_rounding_of_float64(bits, K):
    """w8a8_ref.int_inputs per expert (sums < 2^24, power-of-two scales: exact in fp32 in any order), padded strides"""
    rng = np.random.default_rng(7 + K)
    ids = mx.routing(rng, T, TOPK, E, crowd=True)
    rs = np.exp2(rng.integers(-2, 2, size=T * TOPK)).astype(np.float32)
    for N in mx.SAME_BITS_NS:
        draws = [wr.int_inputs(rng, T * TOPK, K, N) for _ in range(E)]
        aq, asc = draws[0][:2]
        w8, ws = torch.stack([d[2] for d in draws]), torch.stack([d[3] for d in draws])
        w = _padded(w8, ws)
        for a_div in (TOPK, 1):
            rows = T * TOPK // a_div
            want = fref.grouped_fp8_ref(wr.w8_as64(aq[:rows]) * as64(asc[:rows])[:, None], wr.w8_as64(w8), as64(ws),
                                        ids, a_div)
            a = _padded(aq[:rows], asc[:rows])
            for blocks in mx.LAUNCH_BLOCKS[N]:
                lists = _lists(ids, E, blocks)
                assert torch.equal(_run(a, w, lists, a_div, bits).cpu(), rounded(want, bits)), (N, a_div, blocks)
                got = _run(a, w, lists, a_div, bits, row_scale=torch.from_numpy(rs).to(DEV))
                assert torch.equal(got.cpu(), rounded(want * rs[:, None], bits)), (N, a_div, blocks, "row_scale")


@pytest.mark.parametrize("K", [160, 672])
@pytest.mark.parametrize("bits", BITS)
def test_an_experts_rows_are_the_linears_bits_for_every_launch_shape(bits, K):
    rng = np.random.default_rng(11 + K)
    ids = mx.routing(rng, T, TOPK, E, crowd=True)
    a = _random(rng, (T * TOPK,), K, -10, -8)
    for N, silu in [(N, False) for N in mx.SAME_BITS_NS] + [(N, True) for N in mx.SILU_BLOCKS]:
        w = _random(rng, (E, N), K, -6, -4)
        for a_div in (TOPK, 1):
            ar = (a[0][:T * TOPK // a_div], a[1][:T * TOPK // a_div])
            want = _linear_bits(ar, w, ids, N, a_div, silu, bits)
            for blocks in (mx.SILU_BLOCKS if silu else mx.LAUNCH_BLOCKS)[N]:
                got = _run(ar, w, _lists(ids, E, blocks), a_div, bits, silu=silu)
                assert torch.equal(got, want), (N, silu, a_div, blocks)


def test_random_data_against_float64():
    rng, K, N, n_tok, n_exp = np.random.default_rng(3), 672, 160, 70, 8
    ids = mx.routing(rng, n_tok, TOPK, n_exp)
    a, w = _random(rng, (n_tok,), K, -10, -8), _random(rng, (n_exp, N), K, -6, -4)
    want = fref.grouped_fp8_ref(wr.w8_as64(a[0]) * as64(a[1])[:, None], wr.w8_as64(w[0]), as64(w[1]), ids, TOPK)
    assert wr.rel_err(as64(_run(a, w, _lists(ids, n_exp), TOPK, "bf16")), want) <= wr.GEMM_TOL["bf16"]


def test_dead_blocks_and_expert_ids_outside_the_range_leave_their_rows_untouched():
    rng, K, N = np.random.default_rng(5), 160, 64
    ids = mx.routing(rng, T, TOPK, E, crowd=True)
    a, w = _random(rng, (T,), K, -10, -8), _random(rng, (E, N), K, -6, -4)
    srt, eid, npad, n_flat = _lists(ids, E)
    want = _linear_bits(a, w, ids, N, TOPK, False, "bf16")
    assert torch.equal(_run(a, w, (srt, eid, npad, n_flat), TOPK, "bf16"), want)
    n_blocks = int(npad.item()) // 32
    eid2 = torch.cat([torch.tensor([E, -1], dtype=torch.int32, device=DEV), eid[2:]])   # outside [0, E)
    got = _run(a, w, (srt, eid2, npad - 32, n_flat), TOPK, "bf16", complete=False)   # and the last block is dead
    rows = srt.view(-1, 32).cpu().numpy()
    dead = np.intersect1d(np.concatenate([rows[0], rows[1], rows[n_blocks - 1]]), np.arange(n_flat))
    live = np.setdiff1d(np.arange(n_flat), dead)
    assert n_blocks >= 4 and dead.size > 32 and bool(torch.isnan(got[dead]).all())
    assert torch.equal(got[live], want[live])


@pytest.mark.parametrize("bits", BITS)
def test_fused_moe_with_fp8_activations_is_its_kernel_sequence_and_replays(bits):
    from scalellm_amd import kernels, moe
    from scalellm_amd.layers import QuantArgs
    from .test_moe_fp8_cpu import _fp8_state_dict
    dt, cfg = torch_dtype(bits), fref.MOE_LAYER
    H, I, n_exp, k = cfg["hidden"], cfg["intermediate"], cfg["n_experts"], cfg["topk"]
    with pytest.raises(kernels.SlmError, match="fp8"):
        moe.FusedMoE(H, I, n_exp, k, QuantArgs("mxfp4", 4), dtype=dt, device=DEV, act_quant="fp8")
    sd = _fp8_state_dict(H, I, n_exp, scale_form="channel")
    sd["gate.weight"] = sd["gate.weight"].to(dt)

    def make():
        layer = moe.FusedMoE(H, I, n_exp, k, QuantArgs("fp8", 8), dtype=dt, device=DEV, max_tokens=70, router="fused",
                             act_quant="fp8")
        layer.load_state_dict(sd)
        return layer

    layer, g = make(), torch.Generator().manual_seed(1)
    xs = [torch.randn(70, H, generator=g).to(dt).to(DEV) for _ in range(3)]
    ex = layer.experts

    def written_out(x):
        n = x.size(0) * k
        wts, ids = kernels.moe_router(x, layer.gate_weight, k, scoring="softmax", renormalize=True)
        srt, eid = (torch.empty(c, dtype=torch.int32, device=DEV) for c in kernels.moe_align_capacity(n, n_exp, 32))
        npad = torch.zeros(1, dtype=torch.int32, device=DEV)
        kernels.moe_align_block(ids, n_exp, 32, srt, eid, npad)
        act, down = torch.empty(n, I, dtype=dt, device=DEV), torch.empty(n, H, dtype=dt, device=DEV)
        kernels.moe_w8a8_grouped_gemm(*kernels.quantize_fp8_act(x), ex.gate_up, ex.gate_up_scale, act, srt, eid, npad,
                                      k, silu_mul=True)
        kernels.moe_w8a8_grouped_gemm(*kernels.quantize_fp8_act(act), ex.down, ex.down_scale, down, srt, eid, npad, 1,
                                      row_scale=wts.view(-1))
        out = torch.empty(x.size(0), H, dtype=dt, device=DEV)
        kernels.moe_sum(down.view(x.size(0), k, H), out)
        return out

    for n_tok in fref.MOE_TOKENS:
        got = layer(xs[0][:n_tok])
        assert bool(torch.isfinite(got.float()).all()) and float(got.float().abs().max()) > 0
        assert torch.equal(got, written_out(xs[0][:n_tok])), n_tok
    assert torch.equal(layer(xs[1]), make()(xs[1]))                # a second batch through the same buffers
    x, out = xs[0].clone(), torch.empty_like(xs[0])                # every buffer exists: capture allocates nothing
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer(x, out=out)
    for xi in xs:                                                  # the routing changes under the graph
        x.copy_(xi)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, layer(xi)) and torch.equal(out, written_out(xi))
