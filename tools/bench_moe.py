"""FusedMoE (scalellm_amd/moe.py: routing, align, two grouped GEMMs, sum) at Mixtral-8x7B shapes against a host
loop over the experts: per-expert slm_w4a16_gemm calls for int4 experts, torch.matmul for unquantised ones.

    python tools/bench_moe.py [--out profiles/r09_moe.jsonl] [--tokens 1,32,256] [--iters 200]
    python tools/bench_moe.py --dense [--out profiles/r12_moe_dense.jsonl]
    python tools/bench_moe.py --fp8 [--out profiles/r18_moe_fp8.jsonl]
    python tools/bench_moe.py --mxfp4 [--out profiles/r23_moe_mxfp4.jsonl]

hidden 4096, intermediate 14336, E = 8, k = 2, AWQ group 128, bf16 (random weights: 705 MB packed).  One JSON
line per T:
  fused_us        FusedMoE.forward captured once in a hipGraph and replayed `iters` times between device events.
                  Before each replay one of `--pool` different inputs is copied into the static buffer, so the routing
                  -- and with it the experts streamed -- changes from replay to replay and the weights (beyond the
                  256 MB MALL as soon as more than two experts are in use) come from HBM.
  touched_bytes   packed weight + scale bytes of the experts in use (gate_up and down), each counted ONCE, averaged
                  over the pool; streamed_bytes counts an expert once per 32-row block (what the kernel issues when
                  nothing is served from cache).  frac_7tbs = touched_bytes / fused_us over the 7.0 TB/s read ceiling
                  measured in this repository.
  loop_us         the same inputs through the dense kernels: per expert, torch index_select of its tokens,
                  gptq_gemm(gate_up, silu_mul), gptq_gemm(down), scale by the routing weight, index_add_ -- eager,
                  with the routing and the per-expert counts known on the host beforehand (not timed).
  loop_graph_us   that loop for ONE fixed routing captured in a graph (host-known counts can be captured only for a
                  routing that never changes): its best case, without launch gaps.

--dense: the same layer over unquantised bf16 experts (FusedMoE(quant_args=None), slm_moe_gemm; 2.8 GB of weights),
measured the same way; the loop is index_select, torch.matmul (gate | up), SiLU * mul, torch.matmul (down), scale,
index_add_ per expert.

--fp8: the same layer over fp8 (e4m3) experts (FusedMoE(QuantArgs("fp8", 8)), slm_moe_fp8_gemm; 1.4 GB of weights):
the bf16 checkpoint of --dense quantised per output channel by kernels.quantize_fp8_weight, and beside it, in the
same run, the dense bf16 layer over the dequantised weights (the same values, so the same routing and the same
experts streamed).  Both forwards are captured in graphs and replayed over the input pool in `--rounds` alternating
windows of `iters` replays; one JSON line per T with fp8_us / dense_us (the medians; every window is listed),
touched_bytes / streamed_bytes / frac_7tbs over the fp8 bytes (weights + scales), the dense layer's own
dense_frac_7tbs, and fp8_vs_dense_rel_err (different rounding of nothing but the accumulator's scale multiply).

--mxfp4: the same layer over OCP MXFP4 experts (FusedMoE(QuantArgs("mxfp4", 4)), slm_moe_mxfp4_gemm; 0.75 GB of nibbles
and scale bytes): the bf16 checkpoint of --dense quantised by kernels.quantize_mxfp4_weight, and beside it, in the same
process, the fp8 layer of --fp8 over the same bf16 checkpoint and the dense bf16 layer over the dequantised MXFP4
weights (bit-identical output, asserted).  All three forwards are captured and replayed over the input pool in
`--rounds` alternating windows of `iters` replays; one JSON line per T with mxfp4_us / fp8_us / dense_us (the medians;
every window is listed, *_spread = (max - min) / median of the windows), touched_bytes / streamed_bytes / frac_7tbs
over the MXFP4 bytes (nibbles + scale bytes), and the other two layers' own fractions.  The three layers share the
router weights and the inputs, so they route alike and stream the same experts.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalellm_amd import kernels, moe  # noqa: E402
from scalellm_amd.layers import QuantArgs  # noqa: E402

HID, INTER, NE, TOPK, GS = 4096, 14336, 8, 2, 128
READ_CEILING = 7.0e12


def _layer(max_tokens, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    sd = {}
    for e in range(NE):
        for w, (K, N) in (("w1", (HID, INTER)), ("w3", (HID, INTER)), ("w2", (INTER, HID))):
            sd[f"experts.{e}.{w}.qweight"] = torch.randint(-2**31, 2**31 - 1, (K, N // 8), device=dev, generator=g,
                                                           dtype=torch.int64).to(torch.int32)
            sd[f"experts.{e}.{w}.qzeros"] = torch.randint(-2**31, 2**31 - 1, (K // GS, N // 8), device=dev, generator=g,
                                                          dtype=torch.int64).to(torch.int32)
            sd[f"experts.{e}.{w}.scales"] = (torch.rand(K // GS, N, device=dev, generator=g) * 0.015 + 0.005
                                             ).to(torch.bfloat16)
    sd["gate.weight"] = (torch.randn(NE, HID, device=dev, generator=g) * 0.05).to(torch.bfloat16)
    layer = moe.FusedMoE(HID, INTER, NE, TOPK, QuantArgs("awq", 4, GS), scoring="softmax", renormalize=True,
                         max_tokens=max_tokens, dtype=torch.bfloat16, device=dev)
    layer.load_state_dict(sd)
    layer(torch.zeros(1, HID, device=dev, dtype=torch.bfloat16))   # repack + buffers
    return layer


def _dense_layer(max_tokens, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    sd = {}
    for e in range(NE):
        for w, (N, K) in (("w1", (INTER, HID)), ("w3", (INTER, HID)), ("w2", (HID, INTER))):
            sd[f"experts.{e}.{w}.weight"] = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    sd["gate.weight"] = (torch.randn(NE, HID, device=dev, generator=g) * 0.05).to(torch.bfloat16)
    layer = moe.FusedMoE(HID, INTER, NE, TOPK, quant_args=None, scoring="softmax", renormalize=True,
                         max_tokens=max_tokens, dtype=torch.bfloat16, device=dev)
    layer.load_state_dict(sd)
    del sd
    layer(torch.zeros(1, HID, device=dev, dtype=torch.bfloat16))   # stack + buffers
    return layer


def _fp8_and_dense_layers(max_tokens, dev):
    """the --dense checkpoint quantised per output channel, and the dense layer over what the fp8 one computes with"""
    g = torch.Generator(device=dev).manual_seed(0)
    sd8, sd16 = {}, {}
    for e in range(NE):
        for w, (N, K) in (("w1", (INTER, HID)), ("w3", (INTER, HID)), ("w2", (HID, INTER))):
            w8, scale = kernels.quantize_fp8_weight((torch.randn(N, K, device=dev, generator=g) * 0.02
                                                     ).to(torch.bfloat16), "channel")
            sd8[f"experts.{e}.{w}.weight"], sd8[f"experts.{e}.{w}.weight_scale"] = w8, scale
            sd16[f"experts.{e}.{w}.weight"] = (w8.float() * scale[:, None]).to(torch.bfloat16)
    sd8["gate.weight"] = sd16["gate.weight"] = (torch.randn(NE, HID, device=dev, generator=g) * 0.05).to(torch.bfloat16)
    layers = []
    for sd, q in ((sd8, QuantArgs("fp8", 8)), (sd16, None)):
        layer = moe.FusedMoE(HID, INTER, NE, TOPK, quant_args=q, scoring="softmax", renormalize=True,
                             max_tokens=max_tokens, dtype=torch.bfloat16, device=dev)
        layer.load_state_dict(sd)
        sd.clear()
        layer(torch.zeros(1, HID, device=dev, dtype=torch.bfloat16))   # stack + buffers
        layers.append(layer)
    return layers


def _captured(layer, pool, T, dev):
    """layer.forward captured over a static input; returns replay(i) for pool entry i and the static output"""
    x_static, out_static = pool[0].clone(), torch.empty(T, HID, device=dev, dtype=torch.bfloat16)
    eager = layer(pool[1]).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        layer.forward(x_static, out=out_static)
    x_static.copy_(pool[1])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_static, eager), "graph replay differs from the eager forward"

    def replay(i):
        x_static.copy_(pool[i % len(pool)])
        graph.replay()

    return replay, eager


def _main_fp8(args, dev, tokens):
    fp8, dense = _fp8_and_dense_layers(max(tokens), dev)
    ex = fp8.experts
    gu_bytes = (ex.gate_up.numel() + 4 * ex.gate_up_scale.numel()) // NE
    dn_bytes = (ex.down.numel() + 4 * ex.down_scale.numel()) // NE
    dense_bytes = dense.experts.nbytes() // NE
    lines = []
    for T in tokens:
        g = torch.Generator(device=dev).manual_seed(T)
        pool = [torch.randn(T, HID, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(args.pool)]
        run8, y8 = _captured(fp8, pool, T, dev)
        run16, y16 = _captured(dense, pool, T, dev)
        rel = float((y8.float() - y16.float()).abs().mean() / y16.float().abs().mean())
        t8, t16 = [], []
        for _ in range(args.rounds):                    # alternating windows: drift hits both columns alike
            t8.append(_time(run8, args.iters))
            t16.append(_time(run16, args.iters))
        fp8_us, dense_us = sorted(t8)[len(t8) // 2], sorted(t16)[len(t16) // 2]
        routed = [_routing(fp8, x)[1] for x in pool]
        used = [int(ids.unique().numel()) for ids in routed]
        blocks = [int(((torch.bincount(ids.reshape(-1), minlength=NE) + 31) // 32).sum()) for ids in routed]
        n_used, n_blocks = sum(used) / len(used), sum(blocks) / len(blocks)
        touched, streamed = (gu_bytes + dn_bytes) * n_used, (gu_bytes + dn_bytes) * n_blocks
        line = dict(bench="moe_mixtral_8x7b_fp8_bf16", T=T, topk=TOPK, n_experts=NE,
                    fp8_us=round(fp8_us, 2), dense_us=round(dense_us, 2), fp8_over_dense=round(fp8_us / dense_us, 4),
                    fp8_us_windows=[round(t, 2) for t in t8], dense_us_windows=[round(t, 2) for t in t16],
                    experts_in_use=round(n_used, 2), row_blocks=round(n_blocks, 2),
                    touched_bytes=int(touched), streamed_bytes=int(streamed),
                    frac_7tbs=round(touched / (fp8_us * 1e-6) / READ_CEILING, 4),
                    streamed_frac_7tbs=round(streamed / (fp8_us * 1e-6) / READ_CEILING, 4),
                    dense_touched_bytes=int(dense_bytes * n_used),
                    dense_frac_7tbs=round(dense_bytes * n_used / (dense_us * 1e-6) / READ_CEILING, 4),
                    fp8_vs_dense_rel_err=round(rel, 5), iters=args.iters, pool=args.pool, rounds=args.rounds)
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def _mxfp4_fp8_and_dense_layers(max_tokens, dev, sides=("mxfp4", "fp8", "dense")):
    """the --dense checkpoint as MXFP4, as fp8 (per output channel), and the dense layer over the dequantised MXFP4;
    `sides`: which of the three to build (tools/ab_moe_mxfp4_ring.py takes the first alone)"""
    g = torch.Generator(device=dev).manual_seed(0)
    sd4, sd8, sd16 = {}, {}, {}
    for e in range(NE):
        for w, (N, K) in (("w1", (INTER, HID)), ("w3", (INTER, HID)), ("w2", (HID, INTER))):
            key = f"experts.{e}.{w}."
            full = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(torch.bfloat16)
            sd4[key + "weight"], sd4[key + "weight_scale"] = kernels.quantize_mxfp4_weight(full)
            if "fp8" in sides:
                sd8[key + "weight"], sd8[key + "weight_scale"] = kernels.quantize_fp8_weight(full, "channel")
            if "dense" in sides:
                sd16[key + "weight"] = kernels.dequantize_mxfp4_weight(sd4[key + "weight"], sd4[key + "weight_scale"],
                                                                       torch.bfloat16)
            del full
    gate = (torch.randn(NE, HID, device=dev, generator=g) * 0.05).to(torch.bfloat16)
    layers = []
    for side, sd, q in (("mxfp4", sd4, QuantArgs("mxfp4", 4)), ("fp8", sd8, QuantArgs("fp8", 8)), ("dense", sd16, None)):
        if side not in sides:
            continue
        sd["gate.weight"] = gate
        layer = moe.FusedMoE(HID, INTER, NE, TOPK, quant_args=q, scoring="softmax", renormalize=True,
                             max_tokens=max_tokens, dtype=torch.bfloat16, device=dev)
        layer.load_state_dict(sd)
        sd.clear()
        layer(torch.zeros(1, HID, device=dev, dtype=torch.bfloat16))   # stack + buffers
        layers.append(layer)
    return layers


def _main_mxfp4(args, dev, tokens):
    mx4, fp8, dense = _mxfp4_fp8_and_dense_layers(max(tokens), dev)
    mx_bytes, fp8_bytes, dense_bytes = (l.experts.nbytes() // NE for l in (mx4, fp8, dense))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    spread = lambda t: round((max(t) - min(t)) / med(t), 4)  # noqa: E731
    lines = []
    for T in tokens:
        g = torch.Generator(device=dev).manual_seed(T)
        pool = [torch.randn(T, HID, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(args.pool)]
        run4, y4 = _captured(mx4, pool, T, dev)
        run8, y8 = _captured(fp8, pool, T, dev)
        run16, y16 = _captured(dense, pool, T, dev)
        assert torch.equal(y4, y16), "the MXFP4 layer differs from the dense layer on the dequantised experts"
        rel8 = float((y8.float() - y16.float()).abs().mean() / y16.float().abs().mean())
        t4, t8, t16 = [], [], []
        for _ in range(args.rounds):                    # alternating windows: drift hits all columns alike
            t4.append(_time(run4, args.iters))
            t8.append(_time(run8, args.iters))
            t16.append(_time(run16, args.iters))
        mx_us, fp8_us, dense_us = med(t4), med(t8), med(t16)
        routed = [_routing(mx4, x)[1] for x in pool]
        used = [int(ids.unique().numel()) for ids in routed]
        blocks = [int(((torch.bincount(ids.reshape(-1), minlength=NE) + 31) // 32).sum()) for ids in routed]
        n_used, n_blocks = sum(used) / len(used), sum(blocks) / len(blocks)
        frac = lambda nbytes, us: round(nbytes * n_used / (us * 1e-6) / READ_CEILING, 4)  # noqa: E731
        line = dict(bench="moe_mixtral_8x7b_mxfp4_bf16", T=T, topk=TOPK, n_experts=NE,
                    mxfp4_us=round(mx_us, 2), fp8_us=round(fp8_us, 2), dense_us=round(dense_us, 2),
                    mxfp4_over_fp8=round(mx_us / fp8_us, 4), mxfp4_over_dense=round(mx_us / dense_us, 4),
                    mxfp4_us_windows=[round(t, 2) for t in t4], fp8_us_windows=[round(t, 2) for t in t8],
                    dense_us_windows=[round(t, 2) for t in t16],
                    mxfp4_spread=spread(t4), fp8_spread=spread(t8), dense_spread=spread(t16),
                    experts_in_use=round(n_used, 2), row_blocks=round(n_blocks, 2),
                    touched_bytes=int(mx_bytes * n_used), streamed_bytes=int(mx_bytes * n_blocks),
                    frac_7tbs=frac(mx_bytes, mx_us),
                    streamed_frac_7tbs=round(mx_bytes * n_blocks / (mx_us * 1e-6) / READ_CEILING, 4),
                    fp8_frac_7tbs=frac(fp8_bytes, fp8_us), dense_frac_7tbs=frac(dense_bytes, dense_us),
                    mxfp4_equals_dense_on_dequantised=True, fp8_vs_mxfp4_rel_err=round(rel8, 5),
                    iters=args.iters, pool=args.pool, rounds=args.rounds)
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def _routing(layer, x):
    logits = x.float() @ layer.gate_weight.float().t()
    w, ids = kernels.moe_topk_softmax(logits, TOPK, True)
    return w.cpu(), ids.cpu()


def _loop_plan(layer, x, dev):
    """host-known routing -> per expert (token rows, weights), as a dense-kernel host would hold them"""
    w, ids = _routing(layer, x)
    plan = []
    for e in range(NE):
        t, j = (ids == e).nonzero(as_tuple=True)
        if t.numel():
            plan.append((e, t.to(dev), w[t, j].to(dev, torch.bfloat16).unsqueeze(1)))
    return plan


def _loop_forward(layer, x, plan, out):
    out.zero_()
    for e, rows, w in plan:
        xs = x.index_select(0, rows)
        h = torch.empty(xs.size(0), INTER, dtype=x.dtype, device=x.device)
        kernels.gptq_gemm(xs, layer.experts.gate_up.expert(e), h, silu_mul=True)
        d = torch.empty(xs.size(0), HID, dtype=x.dtype, device=x.device)
        kernels.gptq_gemm(h, layer.experts.down.expert(e), d)
        out.index_add_(0, rows, d * w)
    return out


def _loop_forward_dense(layer, x, plan, out):
    out.zero_()
    for e, rows, w in plan:
        xs = x.index_select(0, rows)
        h = torch.matmul(xs, layer.experts.gate_up[e].t())
        act = torch.nn.functional.silu(h[:, :INTER]) * h[:, INTER:]
        out.index_add_(0, rows, torch.matmul(act, layer.experts.down[e].t()) * w)
    return out


def _time(fn, iters):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tokens", default="1,32,256")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--dense", action="store_true", help="unquantised bf16 experts (slm_moe_gemm)")
    ap.add_argument("--fp8", action="store_true",
                    help="fp8 (e4m3) experts (slm_moe_fp8_gemm) beside the dense bf16 layer on the dequantised weights")
    ap.add_argument("--mxfp4", action="store_true",
                    help="MXFP4 experts (slm_moe_mxfp4_gemm) beside the fp8 layer and the dense bf16 layer on the "
                         "dequantised weights")
    ap.add_argument("--rounds", type=int, default=3, help="--fp8 / --mxfp4: alternating timing windows per layer")
    args = ap.parse_args()
    if args.dense + args.fp8 + args.mxfp4 > 1:
        raise SystemExit("--dense, --fp8 and --mxfp4 are three modes: pick one (--fp8 and --mxfp4 measure the dense "
                         "layer too)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda")
    tokens = [int(t) for t in args.tokens.split(",")]
    if args.fp8:
        _write(args.out, _main_fp8(args, dev, tokens))
        return
    if args.mxfp4:
        _write(args.out, _main_mxfp4(args, dev, tokens))
        return
    if args.dense:
        layer = _dense_layer(max(tokens), dev)
        gu_bytes, dn_bytes = layer.experts.gate_up.numel() * 2 // NE, layer.experts.down.numel() * 2 // NE
        loop_forward, name = _loop_forward_dense, "moe_mixtral_8x7b_dense_bf16"
    else:
        layer = _layer(max(tokens), dev)
        gu_bytes, dn_bytes = layer.experts.gate_up.nbytes() // NE, layer.experts.down.nbytes() // NE
        loop_forward, name = _loop_forward, "moe_mixtral_8x7b_awq_g128_bf16"
    per_expert = gu_bytes + dn_bytes
    lines = []
    for T in tokens:
        g = torch.Generator(device=dev).manual_seed(T)
        pool = [torch.randn(T, HID, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(args.pool)]
        x_static, out_static = pool[0].clone(), torch.empty(T, HID, device=dev, dtype=torch.bfloat16)
        eager = layer(pool[1]).clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            layer.forward(x_static, out=out_static)
        x_static.copy_(pool[1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_static, eager), "graph replay differs from the eager forward"

        def fused(i):
            x_static.copy_(pool[i % len(pool)])
            graph.replay()

        fused_us = _time(fused, args.iters)

        plans = [_loop_plan(layer, x, dev) for x in pool]
        out_loop = torch.zeros(T, HID, device=dev, dtype=torch.bfloat16)
        loop_us = _time(lambda i: loop_forward(layer, pool[i % len(pool)], plans[i % len(pool)], out_loop), args.iters)
        # agreement of the two paths on one input (different rounding points: a tolerance, not equality)
        ref = loop_forward(layer, pool[1], plans[1], out_loop).float()
        rel = float((eager.float() - ref).abs().mean() / ref.abs().mean())
        torch.cuda.synchronize()
        lg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(lg):
            loop_forward(layer, x_static, plans[0], out_loop)
        x_static.copy_(pool[0])
        loop_graph_us = _time(lambda i: lg.replay(), args.iters)

        used = [len(p) for p in plans]
        blocks = [sum((rows.numel() + 31) // 32 for _, rows, _ in p) for p in plans]
        touched = per_expert * sum(used) / len(used)
        streamed = (gu_bytes + dn_bytes) * sum(blocks) / len(blocks)
        line = dict(bench=name, T=T, topk=TOPK, n_experts=NE,
                    fused_us=round(fused_us, 2), loop_us=round(loop_us, 2), loop_graph_us=round(loop_graph_us, 2),
                    experts_in_use=round(sum(used) / len(used), 2), row_blocks=round(sum(blocks) / len(blocks), 2),
                    touched_bytes=int(touched), streamed_bytes=int(streamed),
                    frac_7tbs=round(touched / (fused_us * 1e-6) / READ_CEILING, 4),
                    streamed_frac_7tbs=round(streamed / (fused_us * 1e-6) / READ_CEILING, 4),
                    fused_vs_loop_rel_err=round(rel, 5), iters=args.iters, pool=args.pool)
        print(json.dumps(line), flush=True)
        lines.append(line)
    _write(args.out, lines)


def _write(path, lines):
    if path:
        with open(path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
