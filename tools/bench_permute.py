"""MoE token permutation (include/slm_hip.h section 14; csrc/permute.hip) against the torch composition, bf16, under
graph replay, at Mixtral (dim 4096, E 8, k 2) and DeepSeek-V3-like (dim 7168, E 256, k 8) shapes.

    python tools/bench_permute.py [--out profiles/r15_permute.jsonl] [--tokens 1,32,256,4096] [--window 0.3]

One JSON line per (shape, T):
  permute_us / torch_permute_us      routing -> permuted rows.  Ours: slm_permute_index_map + slm_permute_rows.
                                     torch: stable argsort of the flattened ids, // k, index_select.
  unpermute_us / torch_unpermute_us  permuted rows -> tokens.  Ours: slm_unpermute_rows (fp32 probabilities fused).
                                     torch: gather of the probabilities, multiply, zero_ + index_add_.
Each graph holds `--pool` calls over different routings (so per-call launch gaps are inside the graph for both
sides, and no routing repeats back to back); it is replayed until `--window` seconds have passed between two
device events, after a warm-up.  *_bytes are the bytes the operation has to move (rows read + rows written; the
maps and ids are below 1 %), *_tbs = bytes / time, frac_7tbs against the 7.0 TB/s read ceiling measured in this
repository.  A composition that cannot be captured is timed eagerly and flagged torch_graph = false.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalellm_amd import kernels  # noqa: E402

SHAPES = (("mixtral", 4096, 8, 2), ("deepseek_v3", 7168, 256, 8))
READ_CEILING = 7.0e12


def _time(fn, window_s):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    iters = max(10, int(window_s * 1e3 / max(start.elapsed_time(stop), 1e-3)))
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters, iters


def _captured(body, window_s):
    """(microseconds per replay, replays, captured?) of body()"""
    body()
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            body()
    except RuntimeError:
        torch.cuda.synchronize()
        return (*_time(body, window_s), False)
    return (*_time(graph.replay, window_s), True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tokens", default="1,32,256,4096")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of replays per timing")
    ap.add_argument("--pool", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_permute needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda")
    lines = []
    for name, dim, E, k in SHAPES:
        for T in (int(t) for t in args.tokens.split(",")):
            g = torch.Generator(device=dev).manual_seed(T)
            x = torch.randn(T, dim, device=dev, dtype=torch.bfloat16, generator=g)
            pool = []
            for _ in range(args.pool):
                logits = torch.rand(T, E, device=dev, generator=g)
                w, ids = logits.topk(k, dim=-1)
                pool.append((ids.to(torch.int32).contiguous(), torch.softmax(w, -1).contiguous()))
            permuted = torch.empty(T * k, dim, device=dev, dtype=torch.bfloat16)
            out = torch.empty(T, dim, device=dev, dtype=torch.bfloat16)
            maps = [torch.empty(k, T, dtype=torch.int32, device=dev) for _ in pool]

            def ours_permute():
                for (ids, _), rmap in zip(pool, maps):
                    kernels.permute_with_index_map(x, ids, E, out=permuted, row_id_map=rmap)

            def ours_unpermute():
                for (_, probs), rmap in zip(pool, maps):
                    kernels.unpermute_with_index_map(permuted, rmap, probs, out=out)

            orders = [torch.empty(T * k, dtype=torch.int64, device=dev) for _ in pool]

            def torch_permute():
                for (ids, _), order in zip(pool, orders):
                    order.copy_(torch.argsort(ids.view(-1), stable=True))
                    torch.index_select(x, 0, order // k, out=permuted)

            def torch_unpermute():
                for (_, probs), order in zip(pool, orders):
                    p = probs.view(-1)[order].to(torch.bfloat16).unsqueeze(1)
                    out.zero_()
                    out.index_add_(0, order // k, permuted * p)

            p_us, p_n, _ = _captured(ours_permute, args.window)
            ours_rows = permuted.clone()
            u_us, u_n, _ = _captured(ours_unpermute, args.window)
            ours_out = out.clone()
            tp_us, tp_n, tp_graph = _captured(torch_permute, args.window)
            assert torch.equal(permuted, ours_rows), "the two permutes disagree"
            tu_us, tu_n, tu_graph = _captured(torch_unpermute, args.window)
            rel = float((out.float() - ours_out.float()).abs().mean() / ours_out.float().abs().mean())
            row_bytes = dim * 2
            moved = T * row_bytes + T * k * row_bytes                  # the same for both directions
            per = lambda us: us / args.pool  # noqa: E731
            line = dict(bench=f"permute_{name}_bf16", T=T, dim=dim, n_experts=E, topk=k, moved_bytes=moved,
                        permute_us=round(per(p_us), 2), torch_permute_us=round(per(tp_us), 2),
                        unpermute_us=round(per(u_us), 2), torch_unpermute_us=round(per(tu_us), 2),
                        permute_tbs=round(moved / per(p_us) / 1e6, 3), unpermute_tbs=round(moved / per(u_us) / 1e6, 3),
                        permute_frac_7tbs=round(moved / (per(p_us) * 1e-6) / READ_CEILING, 4),
                        unpermute_frac_7tbs=round(moved / (per(u_us) * 1e-6) / READ_CEILING, 4),
                        torch_graph=bool(tp_graph and tu_graph), unpermute_vs_torch_rel_err=round(rel, 5),
                        replays=dict(permute=p_n, unpermute=u_n, torch_permute=tp_n, torch_unpermute=tu_n),
                        pool=args.pool)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del permuted, out, x, ours_rows, ours_out
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
