"""Multi-head latent attention (kernels.mla_paged_kv, csrc/mla.hip) at DeepSeek shapes: head_dim 512 + 64, bf16,
block 64, kv_len 4096.

    python tools/bench_mla.py [--out profiles/r10_mla.jsonl] [--iters 200] [--rows decode,chunked]

Rows: decode (q_len 1) with n_heads in {128, 16} x batch in {1, 32, 128}, and one chunked-prefill row (4 sequences
x 256 query tokens at the end of a 4096-token history, 128 heads).  One JSON line per row:
  us            the replay period, not a kernel time: one call captured in a hipGraph and replayed `iters` times
                between device events, the copy of the next block table (16 KiB at most) in front of each replay
                included.  At batch 1 the window is only 8-11 ms.  The latent cache
                holds 128 x 4096 slots (604 MB, beyond the 256 MB MALL); before each replay the next of `pool` block
                tables is copied into the static table, each pointing at a different region of the cache, so that a
                small batch does not re-read its few megabytes from cache replay after replay.
  cache_bytes   latent + RoPE-key bytes of the tokens the call attends to, each counted ONCE (1152 B per token);
                tbs = cache_bytes / us, frac_7tbs against the 7.0 TB/s read ceiling measured in this repository.
  flop          2 x (576 + 512) per visible (query row, kv token) pair; tflops = flop / us, frac_1p67pf against the
                matrix pipe's sustained 1.67 PFLOP/s (profiles/r03_clock_under_load.jsonl).
  bound         which of the two roofs is the higher floor for this row ("hbm" or "mfma") and roof_us, that floor.
  torch_us      the same call as an eager torch composition: gather by slot, bf16 einsum, softmax in fp32 (the
                baseline r07 / r08 / r09 use), timed over min(iters, 20) calls; its window INCLUDES expanding the block
                table into slot lists (three small kernels per call: arange, int -> long, add);
                rel_err_vs_torch: relative L2 distance of the two outputs.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalellm_amd import kernels  # noqa: E402

HD, ROPE, BLOCK, KV_LEN = 512, 64, 64, 4096
READ_CEILING = 7.0e12
MFMA_SUSTAINED = 1.67e15
CACHE_SEQS = 128  # the cache holds this many 4096-token histories

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


def _torch_mla(q, q_rope, kvc, krc, slots, bs, q_len, sm_scale):
    """gather by slot, bf16 einsum, softmax in fp32; slots [bs, kv_len]"""
    kv, kr = kvc[slots], krc[slots]
    H = q.size(1)
    s = torch.einsum("bqhd,bkd->bhqk", q.view(bs, q_len, H, HD), kv) + \
        torch.einsum("bqhr,bkr->bhqk", q_rope.view(bs, q_len, H, ROPE), kr)
    s = s.float() * sm_scale
    if q_len > 1:
        L = slots.size(1)
        vis = torch.arange(L, device=q.device)[None, :] <= torch.arange(q_len, device=q.device)[:, None] + (L - q_len)
        s = s.masked_fill(~vis, float("-inf"))
    p = torch.softmax(s, dim=-1).to(q.dtype)
    return torch.einsum("bhqk,bkd->bqhd", p, kv).reshape(bs * q_len, H, HD)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--rows", default="decode,chunked")
    ap.add_argument("--heads", default="128,16")
    ap.add_argument("--batches", default="1,32,128")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda")
    dt = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    n_blocks_seq = KV_LEN // BLOCK
    total_blocks = CACHE_SEQS * n_blocks_seq
    kvc = torch.randn(total_blocks * BLOCK, HD, device=dev, generator=g, dtype=torch.float32).to(dt)
    krc = torch.randn(total_blocks * BLOCK, ROPE, device=dev, generator=g, dtype=torch.float32).to(dt)
    sm_scale = 1.0 / (HD + ROPE) ** 0.5
    rows = []
    if "decode" in args.rows:
        rows += [(int(h), int(b), 1) for h in args.heads.split(",") for b in args.batches.split(",")]
    if "chunked" in args.rows:
        rows.append((128, 4, 256))
    kernels.reserve_workspace(256 << 20, dev)
    lines = []
    for H, bs, q_len in rows:
        T = bs * q_len
        q = torch.randn(T, H, HD, device=dev, generator=g, dtype=torch.float32).to(dt)
        qr = torch.randn(T, H, ROPE, device=dev, generator=g, dtype=torch.float32).to(dt)
        out = torch.empty_like(q)
        i32 = dict(dtype=torch.int32, device=dev)
        q_cu = torch.arange(0, T + 1, q_len, **i32)
        kv_cu = torch.arange(0, bs * KV_LEN + 1, KV_LEN, **i32)
        bcu = torch.arange(0, bs * n_blocks_seq + 1, n_blocks_seq, **i32)
        # pool of block tables: table j is a random permutation of the blocks of region j of the cache
        n_pool = max(1, min(args.pool, CACHE_SEQS // bs))
        tables = []
        for j in range(n_pool):
            perm = torch.randperm(bs * n_blocks_seq, device=dev, generator=g) + j * bs * n_blocks_seq
            tables.append((perm * BLOCK).to(torch.int32))
        bt = tables[0].clone()

        def call():
            kernels.mla_paged_kv(out, q, qr, kvc, krc, q_cu, kv_cu, bt, bcu, BLOCK, q_len, KV_LEN, sm_scale)

        call()
        torch.cuda.synchronize()
        eager = out.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), "graph replay differs from the eager call"

        def replay(i):
            bt.copy_(tables[i % n_pool])
            graph.replay()

        us = _time(replay, args.iters)

        def slots_of(tbl):
            return (tbl.long().view(bs, n_blocks_seq, 1) + torch.arange(BLOCK, device=dev)).view(bs, KV_LEN)

        torch_iters = max(3, min(args.iters, 20))
        torch_us = _time(lambda i: _torch_mla(q, qr, kvc, krc, slots_of(tables[i % n_pool]), bs, q_len, sm_scale),
                         torch_iters)
        bt.copy_(tables[0])
        graph.replay()
        ref = _torch_mla(q, qr, kvc, krc, slots_of(tables[0]), bs, q_len, sm_scale).float()
        rel = float((out.float() - ref).norm() / ref.norm())
        del ref
        cache_bytes = bs * KV_LEN * (HD + ROPE) * 2
        pairs = bs * H * sum(KV_LEN - q_len + t + 1 for t in range(q_len))
        flop = 2 * (HD + ROPE + HD) * pairs
        t_hbm, t_mfma = cache_bytes / READ_CEILING * 1e6, flop / MFMA_SUSTAINED * 1e6
        splits = kernels.mla_paged_kv_auto_splits(T, bs, H, HD, q_len, KV_LEN)
        line = dict(bench="mla_paged_kv_bf16_d512_r64_block64", n_heads=H, batch=bs, q_len=q_len, kv_len=KV_LEN,
                    splits=splits, us=round(us, 2), cache_bytes=cache_bytes, tbs=round(cache_bytes / us * 1e-6, 3),
                    frac_7tbs=round(cache_bytes / (us * 1e-6) / READ_CEILING, 4), flop=flop,
                    tflops=round(flop / us * 1e-6, 1), frac_1p67pf=round(flop / (us * 1e-6) / MFMA_SUSTAINED, 4),
                    bound="hbm" if t_hbm >= t_mfma else "mfma", roof_us=round(max(t_hbm, t_mfma), 2),
                    torch_us=round(torch_us, 2), rel_err_vs_torch=round(rel, 5), iters=args.iters, pool=n_pool)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
