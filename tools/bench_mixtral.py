"""The fused MoE router (slm_moe_router, include/slm_hip.h section 17) and the Mixtral decode step, measured three ways.
Everything is captured once in a hipGraph and replayed `--iters` times between device events, in one process;
every figure is the median of `--repeats` such windows, listed with their spread (max - min).

    python tools/bench_mixtral.py [--out profiles/r19_mixtral.jsonl] [--iters 200] [--repeats 5] [--parts router,layer,step]
    python tools/bench_mixtral.py --parts step --quants fp8,mxfp4      # the step rows of profiles/r23_moe_mxfp4.jsonl

  router  kernels.moe_router alone against the captured composition it replaces (x.float() @ gate_f32_t, then the
          section 10 routing kernel): Mixtral rows (E 8, hidden 4096, softmax top 2) and DeepSeek-V3-like rows (E 256,
          hidden 7168, grouped sigmoid 8 groups / 4 kept / top 8), T = 1 / 32 / 256.  `splits` is what
          slm_moe_router_splits plans (this version: always 1, the only form there is).
  layer   FusedMoE(router="fused") against router="torch" at the Mixtral-8x7B layer (hidden 4096, intermediate 14336,
          E 8, k 2) for the three experts classes, T = 1 / 32 / 256, over a pool of inputs (the routing changes from
          replay to replay).
  step    MixtralDecodeStep at the 8x7B shape cut to 8 of its 32 layers, kv 4096, batch 1 and 32, per quant_method
          (--quants, default none,fp8,awq), with the fused router and with the layers' router switched to "torch".
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalellm_amd import kernels, moe  # noqa: E402
from scalellm_amd.decode import make_decode_inputs  # noqa: E402
from scalellm_amd.layers import QuantArgs  # noqa: E402
from scalellm_amd.mixtral import MixtralDecodeStep, MixtralShape  # noqa: E402

BF16 = torch.bfloat16
TOKENS = (1, 32, 256)


def _window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(min(10, iters)):
        fn(i)
    torch.cuda.synchronize()
    start.record()
    for i in range(iters):
        fn(i)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def _measure(fns, args):
    """alternating windows over the candidates (drift hits all alike) -> per candidate (median us, spread us)"""
    t = [[] for _ in fns]
    for _ in range(args.repeats):
        for i, fn in enumerate(fns):
            t[i].append(_window(fn, args.iters))
    return [(round(sorted(v)[len(v) // 2], 2), round(max(v) - min(v), 2)) for v in t]


def _graph(body):
    body()                                     # warm-up: workspaces, lazy repacks
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    return g


# ---- (i) the router alone ---------------------------------------------------------------------------------------------
def part_router(args, dev):
    lines = []
    for name, E, H, k, grouped in (("mixtral", 8, 4096, 2, None), ("deepseek_v3_like", 256, 7168, 8, (8, 4, 2.5))):
        gen = torch.Generator(device=dev).manual_seed(E)
        w = (torch.randn(E, H, device=dev, generator=gen) * 0.05).to(BF16)
        wt32 = w.float().t().contiguous()
        bias = torch.randn(E, device=dev, generator=gen) * 0.1 if grouped else None
        for T in TOKENS:
            x = torch.randn(T, H, device=dev, dtype=BF16, generator=gen)
            wo, io = torch.empty(T, k, device=dev), torch.empty(T, k, device=dev, dtype=torch.int32)
            wc, ic = torch.empty_like(wo), torch.empty_like(io)
            if grouped:
                ng, tg, sf = grouped
                fused = lambda: kernels.moe_router(x, w, k, scoring="grouped_sigmoid", correction_bias=bias,  # noqa: E731
                                                   n_expert_groups=ng, topk_group=tg, scaling_factor=sf, weights=wo,
                                                   indices=io)
                comp = lambda: kernels.moe_grouped_topk_sigmoid(x.float() @ wt32, bias, ng, tg, k, sf, wc, ic)  # noqa: E731
            else:
                fused = lambda: kernels.moe_router(x, w, k, weights=wo, indices=io)  # noqa: E731
                comp = lambda: kernels.moe_topk_softmax(x.float() @ wt32, k, True, wc, ic)  # noqa: E731
            gf, gc = _graph(fused), _graph(comp)
            (f_us, f_sp), (c_us, c_sp) = _measure([lambda i: gf.replay(), lambda i: gc.replay()], args)
            agree = float((io.sort(1).values == ic.sort(1).values).all(1).float().mean())
            line = dict(bench="moe_router", shape=name, T=T, n_experts=E, hidden=H, topk=k,
                        scoring="grouped_sigmoid" if grouped else "softmax",
                        splits=kernels.moe_router_splits(E, H, BF16), router_us=f_us, router_spread_us=f_sp,
                        composition_us=c_us, composition_spread_us=c_sp, router_over_composition=round(f_us / c_us, 3),
                        same_experts_frac=round(agree, 4), iters=args.iters, repeats=args.repeats)
            print(json.dumps(line), flush=True)
            lines.append(line)
    return lines


# ---- (ii) the layer ---------------------------------------------------------------------------------------------------
def _layer_state(quant, dev):
    s = MixtralShape.mixtral_8x7b()
    step = MixtralDecodeStep(dataclasses.replace(s, n_layers=1, vocab=256), 8, 4, 16, quant_method=quant, device=dev,
                             keep_checkpoint=True)
    return s, step.ckpt[0]["moe"]


def part_layer(args, dev):
    lines = []
    for quant, qa in (("none", None), ("fp8", QuantArgs("fp8", 8)), ("awq", QuantArgs("awq", 4, 128))):
        s, sd = _layer_state(quant, dev)
        layers = {}
        for router in ("fused", "torch"):
            layer = moe.FusedMoE(s.hidden, s.intermediate, s.n_experts, s.topk, qa, scoring="softmax",
                                 renormalize=True, max_tokens=max(TOKENS), dtype=BF16, device=dev, router=router)
            layer.load_state_dict(sd)
            layers[router] = layer
        del sd
        # one set of expert tensors serves both layers
        layers["fused"].experts.repack()
        layers["torch"].experts = layers["fused"].experts
        torch.cuda.empty_cache()
        for T in TOKENS:
            gen = torch.Generator(device=dev).manual_seed(T)
            pool = [torch.randn(T, s.hidden, device=dev, dtype=BF16, generator=gen) for _ in range(args.pool)]
            x_static = pool[0].clone()
            outs = {r: torch.empty(T, s.hidden, device=dev, dtype=BF16) for r in layers}
            graphs = {r: _graph(lambda r=r: layers[r].forward(x_static, out=outs[r])) for r in layers}

            def replay(r):
                def fn(i):
                    x_static.copy_(pool[i % len(pool)])
                    graphs[r].replay()
                return fn
            (f_us, f_sp), (t_us, t_sp) = _measure([replay("fused"), replay("torch")], args)
            rel = float((outs["fused"].float() - outs["torch"].float()).abs().mean() /
                        outs["torch"].float().abs().mean())
            line = dict(bench="fused_moe_router", experts=quant, T=T, fused_router_us=f_us, fused_router_spread_us=f_sp,
                        torch_router_us=t_us, torch_router_spread_us=t_sp, fused_over_torch=round(f_us / t_us, 4),
                        out_rel_diff=round(rel, 5), iters=args.iters, repeats=args.repeats, pool=args.pool)
            print(json.dumps(line), flush=True)
            lines.append(line)
        del layers, graphs
        torch.cuda.empty_cache()
    return lines


# ---- (iii) the step ---------------------------------------------------------------------------------------------------
def part_step(args, dev):
    lines = []
    shape = dataclasses.replace(MixtralShape.mixtral_8x7b(), n_layers=8)
    kv_len, block = 4096, 16
    for quant in args.quants.split(","):
        step = None
        for bs in (1, 32):
            tokens, positions, params, n_blocks = make_decode_inputs(bs, kv_len, block, dev, seed=bs, vocab=shape.vocab)
            if step is None:
                nb = make_decode_inputs(32, kv_len, block, dev, vocab=shape.vocab)[3]
                step = MixtralDecodeStep(shape, 32, nb, block, quant_method=quant, device=dev)
                for L in step.layers:
                    for t in L["kv"].get_kv_cache():
                        t.normal_()
                step.reserve_workspaces(32, kv_len)
            res = {}
            for router in ("fused", "torch"):
                for L in step.layers:
                    L["moe"].router = router
                g = _graph(lambda: step.forward(tokens, positions, params))
                res[router] = g
            (f_us, f_sp), (t_us, t_sp) = _measure([lambda i: res["fused"].replay(), lambda i: res["torch"].replay()],
                                                  args)
            for L in step.layers:
                L["moe"].router = "fused"
            line = dict(bench="mixtral_8x7b_step_8_of_32_layers", quant_method=quant, batch=bs, kv_len=kv_len,
                        step_us=f_us, step_spread_us=f_sp, torch_router_step_us=t_us, torch_router_step_spread_us=t_sp,
                        fused_over_torch=round(f_us / t_us, 4), iters=args.iters, repeats=args.repeats)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del res
        del step
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--parts", default="router,layer,step")
    ap.add_argument("--quants", default="none,fp8,awq", help="the step part's quant_method list")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixtral needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda")
    lines = []
    for part in args.parts.split(","):
        lines += {"router": part_router, "layer": part_layer, "step": part_step}[part](args, dev)
        if args.out:                                   # after every part: a later part's failure loses nothing
            with open(args.out, "w") as f:
                for line in lines:
                    f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
