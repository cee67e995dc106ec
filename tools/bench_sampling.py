"""Fused logits processing + sampling (csrc/sampling.hip) vs the torch composition of the reference's
processors and sampler (src/sampling/logits_processor.h:243-277, sampler.cpp:19-70).

    python tools/bench_sampling.py [--out profiles/r07_sampling.jsonl] [--iters 50]

Grid: bs {1, 32, 256} x vocab 128256 x {greedy, temperature, top-k 50 + top-p 0.9, the same + 64
penalised ids + 5 logprobs}; bf16 logits.  One JSON line per point: kernel_us (the fused launch captured
in a hipGraph and replayed `iters` times between CUDA events: no host time), call_us (the same through the
eager Python call, host included), torch_us (the reference's composition on the same logits, eager).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalellm_amd import kernels  # noqa: E402

CONFIGS = ("greedy", "temperature", "topk50_topp0.9", "topk50_topp0.9_pen64_lp5")


def _params(cfg, n, V, dev):
    g = torch.Generator(device=dev).manual_seed(n)
    kw = dict(seeds=torch.arange(n, dtype=torch.int64, device=dev), positions=torch.full((n,), 100, dtype=torch.int32, device=dev))
    if cfg != "greedy":
        kw["do_sample"] = torch.ones(n, dtype=torch.bool, device=dev)
        kw["temperatures"] = torch.full((n,), 0.8, device=dev)
    if cfg.startswith("topk50"):
        kw["top_k"] = torch.full((n,), 50, dtype=torch.int64, device=dev)
        kw["top_p"] = torch.full((n,), 0.9, device=dev)
    if cfg.endswith("pen64_lp5"):
        kw["unique_token_ids"] = torch.stack([torch.randperm(V, device=dev, generator=g)[:64] for _ in range(n)])
        kw["unique_token_counts"] = torch.randint(1, 4, (n, 64), dtype=torch.int32, device=dev, generator=g)
        kw["unique_token_lens"] = torch.full((n,), 64, dtype=torch.int32, device=dev)
        kw["frequency_penalties"] = torch.full((n,), 0.1, device=dev)
        kw["presence_penalties"] = torch.full((n,), 0.1, device=dev)
        kw["repetition_penalties"] = torch.full((n,), 1.1, device=dev)
        kw["logprobs"] = torch.empty(n, device=dev)
        kw["top_logprobs"] = torch.empty(n, 5, device=dev)
        kw["top_tokens"] = torch.empty(n, 5, dtype=torch.int32, device=dev)
    return kw


def _torch_reference(logits, kw):
    """The reference's torch path: detail:: penalties (gather / scatter), temperature, sort-based
    top-k / top-p, softmax + exponential_ + argmax, log_softmax + topk."""
    x = logits
    if "unique_token_ids" in kw:
        ids, cnt = kw["unique_token_ids"], kw["unique_token_counts"]
        s = x.gather(1, ids)
        s = s - cnt * kw["frequency_penalties"][:, None].to(x.dtype)
        s = s - (cnt > 0) * kw["presence_penalties"][:, None].to(x.dtype)
        x = x.scatter(1, ids, s)
        s = x.gather(1, ids)
        p = kw["repetition_penalties"][:, None].to(x.dtype)
        x = x.scatter(1, ids, torch.where(s < 0, s * p, s / p))
    if "temperatures" in kw:
        x = x / kw["temperatures"][:, None].to(x.dtype)
    if "top_k" in kw:
        srt, idx = x.sort(dim=-1, descending=True)
        mask = torch.arange(x.size(-1), device=x.device).expand_as(srt) >= kw["top_k"][:, None]
        srt = srt.masked_fill(mask, -float("inf"))
        ps = srt.softmax(-1)
        srt = srt.masked_fill((ps.cumsum(-1) - ps) > kw["top_p"][:, None], -float("inf"))
        x = srt.gather(-1, idx.argsort())
    probs = torch.softmax(x, -1, dtype=torch.float32)
    if "do_sample" in kw:
        tok = probs.div(torch.empty_like(probs).exponential_(1)).argmax(-1)
    else:
        tok = probs.argmax(-1)
    if "logprobs" in kw:
        lp = torch.log_softmax(x, -1, dtype=torch.float32)
        lp.gather(-1, tok[:, None])
        lp.topk(5, -1)
    return tok


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def _time_graph(fn, iters):
    fn()  # warm-up: workspace, lazy loads
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return _time(g.replay, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--batch", type=int, nargs="*", default=[1, 32, 256])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    V = args.vocab
    lines = []
    for n in args.batch:
        logits = torch.randn(n, V, device=dev, dtype=torch.bfloat16) * 3
        for cfg in CONFIGS:
            kw = _params(cfg, n, V, dev)
            tok = torch.empty(n, dtype=torch.int32, device=dev)
            k_us = _time_graph(lambda: kernels.sample(logits, next_tokens=tok, **kw), args.iters)
            c_us = _time(lambda: kernels.sample(logits, next_tokens=tok, **kw), args.iters)
            t_us = _time(lambda: _torch_reference(logits, kw), max(5, args.iters // 5))
            rec = dict(bench="sampling", bs=n, vocab=V, dtype="bf16", config=cfg, kernel_us=round(k_us, 2), call_us=round(c_us, 2),
                       torch_us=round(t_us, 2), speedup=round(t_us / k_us, 2))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
