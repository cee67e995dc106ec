"""GPU tests of the fused MoE router (include/slm_hip.h section 17, slm_moe_router; csrc/moe_router.hip): the gate GEMM
against a float64 reference (bit for bit on exactly representable inputs, inside the derived fp32 bound on random
ones), the routing against section 10's own kernels run on the router's logits (bit for bit), batch invariance,
strides and tile edges, graph capture, the C++ shim and FusedMoE(router="fused").

The K-split form (splits > 1) is not built: slm_moe_router_splits plans 1 for every shape and there is no knob, so
every case here runs the one form there is."""
import numpy as np
import pytest
import torch

from . import moe_dense_ref as dref
from . import router_ref as rref
from .router_ref import CASES, GROUPED, SOFTMAX_TOPK, as64

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCORINGS = ("softmax", "grouped_sigmoid")


def _bias(E, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(E, generator=g) * 0.1).to(DEV)


def _route(x, w, scoring, bias=None, logits=True, **out):
    """kernels.moe_router with the case table's routing parameters of this E -> (weights, indices, logits_out)"""
    from scalellm_amd import kernels
    E = w.size(0)
    lo = torch.full((x.size(0), E), float("nan"), device=DEV) if logits else None
    if scoring == "softmax":
        wt, idx = kernels.moe_router(x, w, SOFTMAX_TOPK[E], scoring="softmax", renormalize=True, logits_out=lo, **out)
    else:
        ng, tg, k, sf = GROUPED[E]
        wt, idx = kernels.moe_router(x, w, k, scoring="grouped_sigmoid", correction_bias=bias, n_expert_groups=ng,
                                     topk_group=tg, scaling_factor=sf, logits_out=lo, **out)
    return wt, idx, lo


def _section10(logits, E, scoring, bias):
    """the routing entry of section 10 on given logits"""
    from scalellm_amd import kernels
    if scoring == "softmax":
        return kernels.moe_topk_softmax(logits, SOFTMAX_TOPK[E], True)
    ng, tg, k, sf = GROUPED[E]
    return kernels.moe_grouped_topk_sigmoid(logits, bias, ng, tg, k, sf)


def _ids(case):
    T, E, H, dt = case
    return f"T{T}-E{E}-H{H}-{str(dt).split('.')[-1]}"


# ---- 1. exact inputs, zero tolerance --------------------------------------------------------------------------------
@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_exact_inputs_give_the_reference_bits(case, scoring):
    T, E, H, dt = case
    rng = np.random.default_rng(T * 1000 + E + H)
    x, w = rref.exact_inputs(rng, T, E, H, dt)
    bias = _bias(E)
    wt, idx, lo = _route(x.to(DEV), w.to(DEV), scoring, bias)
    want = rref.router_logits(as64(x), as64(w))
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)       # exact in fp32
    assert np.array_equal(as64(lo), want)                                         # ... and bit for bit what we got
    if scoring == "softmax":
        # the selection is on the logits alone: the stable top-k (lower id first among equal logits -- and with
        # multiples of 1 / 32 below a few units most tokens have some)
        _, ri = rref.topk_softmax(want.astype(np.float32), SOFTMAX_TOPK[E], renormalize=True)
        assert np.array_equal(idx.cpu().numpy(), ri)
    w10, i10 = _section10(lo, E, scoring, bias)
    assert torch.equal(idx, i10) and torch.equal(wt, w10)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_built_ties_go_to_the_lower_expert_id(dt):
    from scalellm_amd import kernels
    T, E, H, k = 33, 8, 96, 2
    rng = np.random.default_rng(17)
    x, w = rref.exact_inputs(rng, T, E, H, dt)
    # (a) two experts with identical gate rows: wherever they compete, the lower id comes first
    w[5] = w[2]
    lo = torch.empty(T, E, device=DEV)
    wt, idx = kernels.moe_router(x.to(DEV), w.to(DEV), k, logits_out=lo)
    want = rref.router_logits(as64(x), as64(w))
    assert np.array_equal(as64(lo), want) and np.array_equal(want[:, 5], want[:, 2])
    _, ri = rref.topk_softmax(want.astype(np.float32), k, True)
    assert np.array_equal(idx.cpu().numpy(), ri)
    sel = idx.cpu().numpy()
    assert not ((sel == 5).any(axis=1) & ~(sel == 2).any(axis=1)).any()           # 5 never without 2
    assert ((sel == 2).any(axis=1)).any()
    # (b) the tie falls exactly between rank k and k + 1: expert 0 = 2 u, experts 3 and 6 = u, the others 0.
    # x.u > 0: logits (2a, a, a, 0 ...) -> {0, 3}, 6 ties with 3 and is left out; x.u < 0: the zeros win -> {1, 2};
    # x.u == 0: everything ties -> {0, 1}
    u = w[3].clone()
    w2 = torch.zeros_like(w)
    w2[0], w2[3], w2[6] = 2 * u, u, u
    wt, idx = kernels.moe_router(x.to(DEV), w2.to(DEV), k, logits_out=lo)
    want = rref.router_logits(as64(x), as64(w2))
    assert np.array_equal(as64(lo), want)
    a = want[:, 3]
    expect = np.where((a > 0)[:, None], [0, 3], np.where((a < 0)[:, None], [1, 2], [0, 1])).astype(np.int32)
    assert (a > 0).any() and (a < 0).any()
    assert np.array_equal(idx.cpu().numpy(), expect)
    assert np.array_equal(rref.topk_softmax(want.astype(np.float32), k, True)[1], expect)


# ---- 2. random inputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_random_inputs_meet_the_fp32_bound_and_section_10s_bits(case, scoring):
    T, E, H, dt = case
    rng = np.random.default_rng(7 + T * 1000 + E + H)
    x, w = rref.random_inputs(rng, T, E, H, dt, scale=4.0)
    bias = _bias(E)
    xd, wd = x.to(DEV), w.to(DEV)
    wt, idx, lo = _route(xd, wd, scoring, bias)
    want = rref.router_logits(as64(x), as64(w))
    err = np.abs(as64(lo) - want)
    bound = rref.logit_bound(as64(x), as64(w))
    print(f"{_ids(case)} {scoring}: max err / bound = {float(np.max(err / np.maximum(bound, 1e-300))):.3g}")
    assert (err <= bound).all()
    w10, i10 = _section10(lo, E, scoring, bias)
    assert torch.equal(idx, i10) and torch.equal(wt, w10)
    assert idx.min() >= 0 and idx.max() < E and bool(torch.isfinite(wt).all())
    w2, i2, _ = _route(xd, wd, scoring, bias, logits=False)                       # without logits_out: the same bits
    assert torch.equal(i2, idx) and torch.equal(w2, wt)


# ---- 3. batch invariance ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("E,H,dt", [(64, 512, torch.bfloat16), (8, 96, torch.bfloat16), (256, 4096, torch.bfloat16),
                                    (64, 4096, torch.float16), (8, 4096, torch.bfloat16)])
def test_a_row_routed_alone_gives_the_bits_it_gives_in_the_batch(E, H, dt, scoring):
    T = 70
    rng = np.random.default_rng(E + H)
    x, w = rref.random_inputs(rng, T, E, H, dt, scale=4.0)
    xd, wd, bias = x.to(DEV), w.to(DEV), _bias(E)
    wt, idx, lo = _route(xd, wd, scoring, bias)
    wt2, idx2, lo2 = _route(xd, wd, scoring, bias)
    assert torch.equal(lo, lo2) and torch.equal(wt, wt2) and torch.equal(idx, idx2)   # repeats
    for r in (0, 31, 32, 69):
        w1, i1, l1 = _route(xd[r:r + 1], wd, scoring, bias)
        assert torch.equal(l1[0], lo[r]), r
        assert torch.equal(w1[0], wt[r]) and torch.equal(i1[0], idx[r]), r
    # ... and inside another batch, at another place in its tile
    w3, i3, l3 = _route(xd[27:64], wd, scoring, bias)
    assert torch.equal(l3, lo[27:64]) and torch.equal(w3, wt[27:64]) and torch.equal(i3, idx[27:64])


# ---- 4. strides and edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("T,E,H", [(33, 64, 512), (70, 8, 96), (1, 256, 4096), (5, 64, 32)])
def test_strided_inputs_and_views_inside_poisoned_buffers(T, E, H, scoring):
    from scalellm_amd import kernels
    dt = torch.bfloat16
    rng = np.random.default_rng(T + E + H)
    x, w = rref.exact_inputs(rng, T, E, H, dt)
    nan = float("nan")
    x_wide = torch.full((T + 40, H + 24), nan, device=DEV, dtype=dt)     # rows >= T and columns >= hidden: NaN
    x_wide[:T, :H] = x.to(DEV)
    w_wide = torch.full((E + 3, H + 40), nan, device=DEV, dtype=dt)
    w_wide[:E, :H] = w.to(DEV)
    xv, wv = x_wide[:T, :H], w_wide[:E, :H]
    assert xv.stride(0) > H and wv.stride(0) > H
    k = SOFTMAX_TOPK[E] if scoring == "softmax" else GROUPED[E][2]
    wbuf = torch.full((T + 2, k), nan, device=DEV)
    ibuf = torch.full((T + 2, k), -7, device=DEV, dtype=torch.int32)
    lbuf = torch.full((T + 2, E), nan, device=DEV)
    bias = _bias(E)
    _route(xv, wv, scoring, bias, logits=False, weights=wbuf[1:T + 1], indices=ibuf[1:T + 1])
    if scoring == "softmax":
        kernels.moe_router(xv, wv, k, weights=wbuf[1:T + 1], indices=ibuf[1:T + 1], logits_out=lbuf[1:T + 1])
    else:
        ng, tg, _, sf = GROUPED[E]
        kernels.moe_router(xv, wv, k, scoring=scoring, correction_bias=bias, n_expert_groups=ng, topk_group=tg,
                           scaling_factor=sf, weights=wbuf[1:T + 1], indices=ibuf[1:T + 1], logits_out=lbuf[1:T + 1])
    for buf in (wbuf, lbuf):
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[T + 1]).all())    # the guards are untouched
        assert bool(torch.isfinite(buf[1:T + 1]).all())
    assert bool((ibuf[0] == -7).all()) and bool((ibuf[T + 1] == -7).all())
    assert ibuf[1:T + 1].min() >= 0 and ibuf[1:T + 1].max() < E
    assert np.array_equal(as64(lbuf[1:T + 1]), rref.router_logits(as64(x), as64(w)))
    wt, idx, _ = _route(x.to(DEV), w.to(DEV), scoring, bias)                              # the dense layout
    assert torch.equal(wbuf[1:T + 1], wt) and torch.equal(ibuf[1:T + 1], idx)


# ---- 5. graph capture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scoring", SCORINGS)
def test_a_captured_call_replays_bit_identically_over_new_inputs(scoring):
    T, E, H, dt = 33, 64, 512, torch.bfloat16
    rng = np.random.default_rng(5)
    _, w = rref.random_inputs(rng, T, E, H, dt, scale=4.0)
    wd, bias = w.to(DEV), _bias(E)
    xs = [rref.random_inputs(rng, T, E, H, dt)[0].to(DEV) for _ in range(3)]
    eager = [_route(x, wd, scoring, bias) for x in xs]
    k = eager[0][0].size(1)
    x_static = xs[0].clone()
    ws, is_, ls = (torch.empty(T, k, device=DEV), torch.empty(T, k, device=DEV, dtype=torch.int32),
                   torch.empty(T, E, device=DEV))
    from scalellm_amd import kernels
    kw = dict(weights=ws, indices=is_, logits_out=ls)
    if scoring != "softmax":
        ng, tg, _, sf = GROUPED[E]
        kw.update(scoring=scoring, correction_bias=bias, n_expert_groups=ng, topk_group=tg, scaling_factor=sf)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kernels.moe_router(x_static, wd, k, **kw)
    for x, (wt, idx, lo) in zip(xs, eager):
        x_static.copy_(x)
        graph.replay()
        assert torch.equal(ws, wt) and torch.equal(is_, idx) and torch.equal(ls, lo)
    torch.cuda.synchronize()


# ---- 6. the C++ shim --------------------------------------------------------------------------------------------------
def test_shim_router_matches_the_ctypes_path():
    from scalellm_amd.cpp_host import load_shim
    shim = load_shim()
    T, E, H, dt = 33, 64, 512, torch.bfloat16
    rng = np.random.default_rng(12)
    x, w = rref.random_inputs(rng, T, E, H, dt, scale=4.0)
    xd, wd, bias = x.to(DEV), w.to(DEV), _bias(E)
    for scoring in SCORINGS:
        wt, idx, lo = _route(xd, wd, scoring, bias)
        w2, i2, l2 = torch.zeros_like(wt), torch.zeros_like(idx), torch.zeros_like(lo)
        if scoring == "softmax":
            shim.moe_router(xd, wd, w2, i2, "softmax", True, logits_out=l2)
        else:
            ng, tg, _, sf = GROUPED[E]
            shim.moe_router(xd, wd, w2, i2, scoring, True, bias, ng, tg, sf, l2)
        assert torch.equal(w2, wt) and torch.equal(i2, idx) and torch.equal(l2, lo)


# ---- 7. the layer -----------------------------------------------------------------------------------------------------
HID, INTER, NE, TOPK = 256, 512, 8, 2


def _layer(scoring, router, max_tokens=33, seed=0):
    from scalellm_amd import moe
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for e in range(NE):
        sd[f"experts.{e}.w1.weight"] = (torch.randn(INTER, HID, generator=g) / 16).to(dt)
        sd[f"experts.{e}.w3.weight"] = (torch.randn(INTER, HID, generator=g) / 16).to(dt)
        sd[f"experts.{e}.w2.weight"] = (torch.randn(HID, INTER, generator=g) / 16).to(dt)
    sd["gate.weight"] = (torch.randn(NE, HID, generator=g) * 0.5).to(dt)
    sd["gate.e_score_correction_bias"] = torch.randn(NE, generator=g) * 0.1
    layer = moe.FusedMoE(HID, INTER, NE, TOPK, quant_args=None, scoring=scoring, renormalize=True, n_expert_groups=4,
                         topk_group=2, scaling_factor=1.5, max_tokens=max_tokens, dtype=dt, device=DEV, router=router)
    layer.load_state_dict(sd)
    return layer, sd


@pytest.mark.parametrize("scoring", SCORINGS)
def test_fused_moe_with_the_fused_router(scoring):
    from scalellm_amd import kernels
    T = 33
    layer, sd = _layer(scoring, "fused")
    x = torch.randn(T, HID, device=DEV, dtype=torch.bfloat16, generator=torch.Generator(device=DEV).manual_seed(4))
    logits = torch.empty(T, NE, device=DEV)
    y = layer.forward(x, router_logits_out=logits)
    assert layer._gate_f32_t is None                                   # the fp32 transposed copy is never built
    # by hand: the router, then the existing align / GEMM / sum
    kw = {} if scoring == "softmax" else dict(correction_bias=layer.correction_bias, n_expert_groups=4, topk_group=2,
                                              scaling_factor=1.5)
    l2 = torch.empty_like(logits)
    wt, ids = kernels.moe_router(x, layer.gate_weight, TOPK, scoring=scoring, renormalize=True, logits_out=l2, **kw)
    assert torch.equal(l2, logits)
    n_flat = T * TOPK
    mp, mb = kernels.moe_align_capacity(n_flat, NE, kernels.MOE_GEMM_BLOCK)
    i32 = dict(dtype=torch.int32, device=DEV)
    srt, eid, npad = torch.empty(mp, **i32), torch.empty(mb, **i32), torch.zeros(1, **i32)
    kernels.moe_align_block(ids, NE, kernels.MOE_GEMM_BLOCK, srt, eid, npad)
    act = torch.empty(n_flat, INTER, device=DEV, dtype=x.dtype)
    down = torch.empty(n_flat, HID, device=DEV, dtype=x.dtype)
    kernels.moe_grouped_gemm(x, layer.experts.gate_up, act, srt, eid, npad, TOPK, silu_mul=True)
    kernels.moe_grouped_gemm(act, layer.experts.down, down, srt, eid, npad, 1, row_scale=wt.view(-1))
    want = torch.empty_like(x)
    kernels.moe_sum(down.view(T, TOPK, HID), want)
    assert torch.equal(y, want)
    # the fp64 composition fed the GPU's own routing, at tests/test_moe_dense_gpu.py's tolerance
    rnd = lambda v: dref.as64(dref.rounded(v, "bf16"))  # noqa: E731
    dense = {key: dref.as64(v) for key, v in sd.items() if key.startswith("experts.")}
    x64, w_np, i_np = dref.as64(x), wt.cpu().numpy(), ids.cpu().numpy()
    ref_out = np.zeros((T, HID))
    for t in range(T):
        for j in range(TOPK):
            e = int(i_np[t, j])
            gate, up = rnd(dense[f"experts.{e}.w1.weight"] @ x64[t]), rnd(dense[f"experts.{e}.w3.weight"] @ x64[t])
            a = rnd(gate / (1 + np.exp(-gate)) * up)
            ref_out[t] += rnd(np.float64(w_np[t, j]) * (dense[f"experts.{e}.w2.weight"] @ a))
    err = dref.rel_err(dref.as64(y), rnd(ref_out))
    assert err < 2 * dref.GEMM_TOL["bf16"], err
    # one captured replay against eager
    x_static, out_static = x.clone(), torch.empty_like(x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer.forward(x_static, out=out_static)
    x2 = torch.randn(T, HID, device=DEV, dtype=torch.bfloat16, generator=torch.Generator(device=DEV).manual_seed(5))
    want2 = layer(x2).clone()
    x_static.copy_(x2)
    graph.replay()
    assert torch.equal(out_static, want2) and not torch.equal(want2, y)
    torch.cuda.synchronize()


def test_router_logits_out_needs_the_fused_router():
    from scalellm_amd.kernels import SlmError
    layer, _ = _layer("softmax", "torch")
    x = torch.zeros(2, HID, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(SlmError):
        layer.forward(x, router_logits_out=torch.empty(2, NE, device=DEV))
