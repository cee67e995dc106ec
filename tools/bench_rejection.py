"""Fused rejection sampling (csrc/rejection.hip) vs the eager torch composition of the reference's
RejectionSampler::forward (src/speculative/rejection_sampler.cpp:22-226).

    python tools/bench_rejection.py [--out profiles/r08_rejection.jsonl] [--iters 50]

Grid: bs {1, 32, 256} x k {1, 4, 8} x vocab 128256, bf16 target logits, fp32 draft probabilities, masked
output; {all greedy, all sampled, mixed} x {no logprobs, 5 top logprobs}.  One JSON line per point:
kernel_us (the two launches captured in a hipGraph and replayed `iters` times between CUDA events),
torch_us (the reference's composition on the same inputs, eager, its host syncs included), and bytes /
frac_8tbs: the bytes the call must move (every launch-1 row read once, plus one target and one draft row
per raced row: all sampled sequences are counted as rejecting, an upper bound) over kernel time, as a
fraction of 8 TB/s.  Every replay reads the same inputs: below about 256 MB (bs 1 and 32) they stay in
the MALL between replays, so those rates are not HBM rates.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalellm_amd import kernels  # noqa: E402

MODES = ("greedy", "sampled", "mixed")


def _inputs(n, k, V, mode, dev):
    g = torch.Generator(device=dev).manual_seed(n * 100 + k)
    target = (torch.randn(n, k + 1, V, device=dev, generator=g) * 3).to(torch.bfloat16)
    draft = torch.softmax(target[:, :k].float() + torch.randn(n, k, V, device=dev, generator=g), -1)
    ids = draft.argmax(-1).int()
    bonus = torch.randint(0, V, (n,), device=dev, generator=g, dtype=torch.int32)
    if mode == "greedy":
        do = torch.zeros(n, dtype=torch.bool, device=dev)
    elif mode == "sampled":
        do = torch.ones(n, dtype=torch.bool, device=dev)
    else:
        do = torch.arange(n, device=dev) % 2 == 0
    return target, draft, ids, bonus, do


def _build_accepted_mask(accepted):
    n, k = accepted.shape
    comb = torch.cat([accepted.long(), torch.zeros(n, 1, dtype=torch.long, device=accepted.device)], -1)
    first = (1 - comb).argmax(1, keepdim=True)
    return torch.arange(k + 1, device=accepted.device).unsqueeze(0) <= first


def _torch_reference(ids, draft, target, bonus, do, n_top):
    """RejectionSampler(do_sample, ...).forward(..., mask_out_rejected_tokens=True) as the reference builds it."""
    all_random, all_greedy = bool(do.all().item()), not bool(do.any().item())  # the constructor's host syncs
    tp = torch.softmax(target, -1, dtype=torch.float32)[:, :-1]
    b = bonus.view(-1, 1).long()
    ids = ids.long()

    def greedy():
        t = tp.argmax(-1)
        out = torch.cat([t, b], -1)
        m = _build_accepted_mask(t == ids)
        return out, torch.where(m, out, -torch.ones_like(out))

    def random():
        u = torch.rand(ids.shape, device=ids.device)
        sd = draft.gather(-1, ids.unsqueeze(-1)).squeeze(-1)
        st = tp.gather(-1, ids.unsqueeze(-1)).squeeze(-1)
        acc = u < st / sd
        rec = (tp - draft).clamp_min_(0)
        rec.div_(rec.sum(-1, keepdim=True).clamp_min_(1e-6))
        rt = rec.div_(torch.empty_like(rec).exponential_(1)).argmax(-1)
        out = torch.cat([torch.where(acc, ids, rt), b], -1)
        m = _build_accepted_mask(acc)
        return out, torch.where(m, out, -torch.ones_like(out))

    if all_greedy:
        out, masked = greedy()
    elif all_random:
        out, masked = random()
    else:
        (r, mr), (g, mg) = random(), greedy()
        d = do.view(-1, 1)
        out, masked = torch.where(d, r, g), torch.where(d, mr, mg)
    if n_top:
        lp = torch.log_softmax(target, -1, dtype=torch.float32)
        lp.gather(-1, out.unsqueeze(-1))
        lp.topk(n_top, -1)
    return masked


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
    ap.add_argument("--k", type=int, nargs="*", default=[1, 4, 8])
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition (profiling runs)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    V = args.vocab
    lines = []
    for n in args.batch:
        for k in args.k:
            for mode in MODES:
                target, draft, ids, bonus, do = _inputs(n, k, V, mode, dev)
                seeds = torch.arange(n, dtype=torch.int64, device=dev)
                pos = torch.full((n,), 100, dtype=torch.int32, device=dev)
                n_samp = int(do.sum())
                for n_top in (0, 5):
                    out = dict(next_tokens=torch.empty(n, k + 1, dtype=torch.int32, device=dev),
                               accepted_lens=torch.empty(n, dtype=torch.int32, device=dev))
                    if n_top:
                        out.update(logprobs=torch.empty(n, k + 1, device=dev),
                                   top_logprobs=torch.empty(n, k + 1, n_top, device=dev),
                                   top_tokens=torch.empty(n, k + 1, n_top, dtype=torch.int32, device=dev))

                    def call():
                        kernels.rejection_sample(ids, draft, target, bonus, mask_out_rejected=True, do_sample=do,
                                                 seeds=seeds, positions=pos, **out)
                    k_us = _time_graph(call, args.iters)
                    rows1 = k + (1 if n_top else 0)
                    raced = n_samp * (k if n_top else 1)
                    nbytes = n * rows1 * V * 2 + raced * V * (2 + 4)
                    rec = dict(bench="rejection", bs=n, k=k, vocab=V, dtype="bf16", mode=mode, top_logprobs=n_top,
                               masked=True, kernel_us=round(k_us, 2), bytes=nbytes,
                               tbs=round(nbytes / k_us / 1e6, 3), frac_8tbs=round(nbytes / k_us / 1e6 / 8.0, 3))
                    if not args.no_torch:
                        t_us = _time(lambda: _torch_reference(ids, draft, target, bonus, do, n_top),
                                     max(3, args.iters // 10))
                        rec.update(torch_us=round(t_us, 2), speedup=round(t_us / k_us, 2))
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
                del target, draft
                torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
