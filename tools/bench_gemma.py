"""The Gemma kernels (csrc/gemma.hip) and the Gemma-2 step against their own compositions.

    python tools/bench_gemma.py [--out profiles/r13_gemma2.jsonl] [--iters 200]
                                [--rows sandwich,soft_cap,step,attn_window]

Every time is a replay period, not a kernel time: the work captured in a hipGraph and replayed `iters` times between
device events, after a warm-up of the same replays; the MEDIAN of `windows` such windows is reported, with the
smallest and largest beside it (spread).  One JSON line per row:
  sandwich   slm_gemma_norm form B (post norm + residual + pre norm, one launch) against its own composition from
             single ops -- form A, torch add, form A: three launches -- at hidden 2304 / 3584 / 4608 and T 1 / 32 /
             256, input "x" (a T tensor) or "slabs4" / "slabs8" (fp32 split-K slabs of a deferred GEMM; the
             composition then first reduces them, torch sum + cast, as a GEMM's own reduce kernel would have).
             A graph holds `chain` calls on `chain` different buffer sets, so a replay is long enough to time;
             fused_us / composed_us are per call.  bytes: what form B must move (x or the slabs, the residual in
             and out, out, two weights); fused_tbs from it.
  soft_cap   slm_soft_cap in place on [256, 256000] bf16 against the reference's three element-wise torch ops
             (tanh(x / cap) * cap: three launches, three roundings); bytes = one read + one write.
  step       Gemma2DecodeStep of Gemma-2-9B's shape (hidden 3584, 16 heads x 256, 8 KV heads, intermediate 14336,
             vocab 256000, AWQ g128, bf16) with `layers` of its 42 layers (the KV cache of all 42 at batch 256 and
             4096 tokens would be 360 GB), batch 32 and 256, kv_len 4096, block 16, embedding, lm_head, soft cap and
             greedy argmax included.  The same step with half the layers gives ms_per_layer (the difference over
             the layers dropped), embed_head_argmax_ms (what is left) and ms_42_layers_extrapolated -- an
             extrapolation, not a measurement.
  attn_window  kernels.paged_decode_attention of Gemma-2-9B's attention (16 query heads on 8 KV heads x 256, soft cap
             50, bf16, block 16) with sliding_window 4096 at context 4096 and at context 32768, batch 1 / 8 / 32:
             the pages in front of the window are not read, so the two should take about the same time
             (ratio_32k_over_4k); full_32k_us is the same call without the window, which reads all of them.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalellm_amd import kernels  # noqa: E402

EPS = 1e-6


def _graph_us(fn, iters, windows):
    """median / min / max over `windows` of the replay period in microseconds of fn() captured once"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    for _ in range(max(3, iters // 10)):
        graph.replay()
    torch.cuda.synchronize()
    periods = []
    for _ in range(windows):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            graph.replay()
        stop.record()
        torch.cuda.synchronize()
        periods.append(start.elapsed_time(stop) * 1e3 / iters)
    return statistics.median(periods), min(periods), max(periods)


def _emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def bench_sandwich(args, dev):
    dt, chain = torch.bfloat16, args.chain
    for hidden in (2304, 3584, 4608):
        post = (0.3 * torch.randn(hidden, device=dev)).to(dt)
        pre = (0.3 * torch.randn(hidden, device=dev)).to(dt)
        for T in (1, 32, 256):
            for src in ("x", "slabs4", "slabs8"):
                n_splits = int(src[5:]) if src != "x" else 0
                sets = []
                for _ in range(chain):
                    s = dict(x=(3 * torch.randn(T, hidden, device=dev)).to(dt),
                             res=torch.randn(T, hidden, device=dev).to(dt), out=torch.empty(T, hidden, device=dev, dtype=dt),
                             y=torch.empty(T, hidden, device=dev, dtype=dt))
                    if n_splits:
                        s["slabs"] = torch.randn(n_splits, T, hidden, device=dev)
                        s["handle"] = kernels.DeferredPartials.from_slabs(s["slabs"])
                    sets.append(s)

                def fused():
                    for s in sets:
                        kernels.gemma_sandwich_norm(s["out"], s["x"], post, s["res"], pre, EPS,
                                                    partials=s.get("handle"))

                def composed():
                    for s in sets:
                        x = s["slabs"].sum(0).to(dt) if n_splits else s["x"]
                        kernels.gemma_rms_norm(s["y"], x, post, EPS)
                        s["res"].add_(s["y"])
                        kernels.gemma_rms_norm(s["out"], s["res"], pre, EPS)

                f = [v / chain for v in _graph_us(fused, args.iters, args.windows)]
                c = [v / chain for v in _graph_us(composed, args.iters, args.windows)]
                nbytes = T * hidden * (4 * n_splits if n_splits else 2) + 3 * T * hidden * 2 + 2 * hidden * 2
                _emit(dict(row="sandwich", hidden=hidden, T=T, input=src, chain=chain, iters=args.iters,
                           windows=args.windows, fused_us=round(f[0], 3), fused_us_min_max=[round(f[1], 3), round(f[2], 3)],
                           composed_us=round(c[0], 3), composed_us_min_max=[round(c[1], 3), round(c[2], 3)],
                           speedup=round(c[0] / f[0], 3), bytes=nbytes, fused_tbs=round(nbytes / f[0] * 1e-6, 4)),
                      args.out)


def bench_soft_cap(args, dev):
    rows, vocab, cap = 256, 256000, 30.0
    x = (12 * torch.randn(rows, vocab, device=dev)).to(torch.bfloat16)
    y = x.clone()
    f = _graph_us(lambda: kernels.soft_cap(y, cap), args.iters, args.windows)
    c = _graph_us(lambda: torch.tanh(x / cap) * cap, args.iters, args.windows)
    nbytes = 2 * rows * vocab * 2
    _emit(dict(row="soft_cap", rows=rows, vocab=vocab, cap=cap, iters=args.iters, windows=args.windows,
               fused_us=round(f[0], 2), fused_us_min_max=[round(f[1], 2), round(f[2], 2)], composed_us=round(c[0], 2),
               composed_us_min_max=[round(c[1], 2), round(c[2], 2)], speedup=round(c[0] / f[0], 3), bytes=nbytes,
               fused_tbs=round(nbytes / f[0] * 1e-6, 3)), args.out)


def bench_step(args, dev):
    import dataclasses

    from scalellm_amd.decode import make_decode_inputs
    from scalellm_amd.gemma2 import Gemma2DecodeStep, Gemma2Shape
    kv_len, block = 4096, 16
    for bs in (32, 256):
        ms = {}
        for layers in (args.layers, args.layers // 2):
            shape = dataclasses.replace(Gemma2Shape.gemma2_9b(), n_layers=layers)
            tokens, positions, params, n_blocks = make_decode_inputs(bs, kv_len, block, dev, seed=1, vocab=shape.vocab)
            model = Gemma2DecodeStep(shape, bs, n_blocks, block, dtype=torch.bfloat16, device=dev, seed=1)
            for L in model.layers:
                for t in L["kv"].get_kv_cache():
                    t.normal_()
            model.reserve_workspaces(bs, kv_len)
            ms[layers] = _graph_us(lambda: model.forward(tokens, positions, params), args.step_iters, args.windows)
            del model
            torch.cuda.empty_cache()
        full, half = ms[args.layers], ms[args.layers // 2]
        per_layer = (full[0] - half[0]) / (args.layers - args.layers // 2)
        _emit(dict(row="step", shape="gemma2_9b", layers=args.layers, bs=bs, kv_len=kv_len, block=block,
                   iters=args.step_iters, windows=args.windows, step_ms=round(full[0] / 1e3, 4),
                   step_ms_min_max=[round(full[1] / 1e3, 4), round(full[2] / 1e3, 4)],
                   half_layers_step_ms=round(half[0] / 1e3, 4), ms_per_layer=round(per_layer / 1e3, 4),
                   embed_head_argmax_ms=round((full[0] - args.layers * per_layer) / 1e3, 4),
                   ms_42_layers_extrapolated=round((full[0] + (42 - args.layers) * per_layer) / 1e3, 3)), args.out)


def bench_attn_window(args, dev):
    from scalellm_amd.decode import make_decode_inputs
    H, HKV, D, block, window, cap = 16, 8, 256, 16, 4096, 50.0
    for bs in (1, 8, 32):
        us = {}
        for ctx, win in ((4096, window), (32768, window), (32768, 0)):
            _, _, p, n_blocks = make_decode_inputs(bs, ctx, block, dev, seed=2)
            q = torch.randn(bs, H, D, device=dev).to(torch.bfloat16)
            kc = torch.randn(n_blocks * block, HKV, D, device=dev).to(torch.bfloat16)
            vc = torch.randn(n_blocks * block, HKV, D, device=dev).to(torch.bfloat16)
            out = torch.empty_like(q)
            us[(ctx, win)] = _graph_us(lambda: kernels.paged_decode_attention(
                out, q, kc, vc, p.kv_cu_seq_lens, p.block_tables, p.cu_block_lens, block, ctx, logit_softcap=cap,
                sliding_window=win), args.iters, args.windows)
            del kc, vc
            torch.cuda.empty_cache()
        w4k, w32k, full = us[(4096, window)], us[(32768, window)], us[(32768, 0)]
        nbytes = 2 * bs * window * HKV * D * 2
        _emit(dict(row="attn_window", heads=[H, HKV, D], bs=bs, window=window, cap=cap, block=block, iters=args.iters,
                   windows=args.windows, ctx_4k_us=round(w4k[0], 2),
                   ctx_4k_us_min_max=[round(w4k[1], 2), round(w4k[2], 2)],
                   ctx_32k_us=round(w32k[0], 2), ctx_32k_us_min_max=[round(w32k[1], 2), round(w32k[2], 2)],
                   ratio_32k_over_4k=round(w32k[0] / w4k[0], 3), full_32k_us=round(full[0], 2),
                   window_bytes=nbytes, ctx_32k_tbs=round(nbytes / w32k[0] * 1e-6, 3)), args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--chain", type=int, default=8, help="sandwich calls (on different buffers) per captured graph")
    ap.add_argument("--layers", type=int, default=8, help="layers of the 9B-shaped step")
    ap.add_argument("--rows", default="sandwich,soft_cap,step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemma needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    rows = args.rows.split(",")
    if "sandwich" in rows:
        bench_sandwich(args, dev)
    if "soft_cap" in rows:
        bench_soft_cap(args, dev)
    if "step" in rows:
        bench_step(args, dev)
    if "attn_window" in rows:
        bench_attn_window(args, dev)


if __name__ == "__main__":
    main()
