"""fp8 (e4m3) KV cache against the bf16 cache -> profiles/r29_attn_fp8.jsonl.

    python tools/bench_attn_fp8.py [--sections attn,append,step] [--reps 15]

attn:   kernels.paged_kv_fp8_attention against kernels.paged_kv_varlen_mha on a bf16 cache of the same shape (q_len 1,
        kv 4096, head_dim 128): 32 / 8 heads at batch 1 / 32 / 128 / 256 and 64 / 8 heads (where the bf16 plan prefers
        its tile kernel) at batch 32 / 128.  Each arm is a captured graph of one call per cache copy, the copies rotating
        over >= 1 GiB so that no call finds its rows in a cache; arms interleaved, three graphs per arm, the median of
        their medians and their spread.  TB/s is K + V bytes of the arm's own cache over its time, `frac` that over the
        7.0 TB/s read ceiling of profiles/r03_clock_under_load.jsonl.
append: RoPE + the quantising append (two launches) against the fused RoPE + append into a bf16 cache (one).
step:   the LlamaDecodeStep 8-of-32-layer step (AWQ int4 linears, kv 4096) at bs 1 / 32 / 128, kv_cache_dtype "fp8"
        against "auto", both pinned to one lane.

Every section runs in a child process of its own under a time limit; the first that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ_CEILING = 7.0e12
ROTATE_BYTES = 1 << 30
KV, BLOCK, D = 4096, 16, 128


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def _capture(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def _time_arms(arms, reps, calls):
    """arms: name -> three graphs of `calls` calls each; interleaved replays.  name -> (median us per call, spread of
    the three graphs' medians)"""
    import torch
    flat = {(n, i): g for n, gs in arms.items() for i, g in enumerate(gs)}
    for g in flat.values():
        for _ in range(2):
            g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in flat}
    for _ in range(reps):
        for k, g in flat.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    out = {}
    for n in arms:
        meds = [_median(times[(n, i)]) for i in range(len(arms[n]))]
        out[n] = (_median(meds), max(meds) - min(meds))
    return out


def run_attn(reps, emit):
    import torch
    from scalellm_amd import kernels
    from scalellm_amd.decode import make_decode_inputs
    dev, dt = "cuda", torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(1)
    for H, KVH, bs in ((32, 8, 1), (32, 8, 32), (32, 8, 128), (32, 8, 256), (64, 8, 32), (64, 8, 128)):
        _, _, prm, n_blocks = make_decode_inputs(bs, KV, BLOCK, dev, seed=3)
        n_slots, row = n_blocks * BLOCK, KVH * D
        kv_elems = 2 * bs * KV * row                                  # K + V elements one call streams
        copies = min(128, max(2, -(-ROTATE_BYTES // kv_elems)))      # sized by the fp8 arm: both arms rotate over >= 1 GiB
        blk = torch.randn(min(n_slots, 1 << 14), KVH, D, device=dev, generator=gen).to(dt)
        rep = -(-n_slots // blk.size(0))
        c16 = [tuple(blk.roll(7 * i + j, 0).repeat(rep, 1, 1)[:n_slots].contiguous() for j in (0, 3)) for i in range(copies)]
        ks, vs = torch.full((KVH,), 0.02, device=dev), torch.full((KVH,), 0.03, device=dev)
        c8 = [(kernels.quantize_fp8_kv(k, ks).view(torch.uint8), kernels.quantize_fp8_kv(v, vs).view(torch.uint8))
              for k, v in c16]
        q = torch.randn(bs, H, D, device=dev, generator=gen).to(dt)
        out = torch.empty_like(q)
        tabs = (prm.q_cu_seq_lens, prm.kv_cu_seq_lens, prm.block_tables, prm.cu_block_lens)

        def bf16():
            for k, v in c16:
                kernels.paged_kv_varlen_mha(out, q, k, v, *tabs, None, BLOCK, 1, KV, D ** -0.5, total_kv_len=bs * KV)

        def fp8():
            for k, v in c8:
                kernels.paged_kv_fp8_attention(out, q, k, v, *tabs, None, BLOCK, 1, KV, D ** -0.5, ks, vs)
        plan = kernels.paged_kv_fp8_attention_plan(out, q, *c8[0], *tabs, None, BLOCK, 1, KV, D ** -0.5, ks, vs)
        bf16_kernel = kernels.paged_kv_varlen_mha_decode_kernel(bs, bs, H, KVH, D, BLOCK, 1, KV)
        us = _time_arms({"bf16": [_capture(bf16) for _ in range(3)], "fp8": [_capture(fp8) for _ in range(3)]}, reps, copies)
        for arm, (t, spread) in us.items():
            nbytes = kv_elems * (2 if arm == "bf16" else 1)
            rec = dict(kind="attn", heads=H, kv_heads=KVH, head_dim=D, bs=bs, kv_len=KV, arm=arm, us=round(t, 2),
                       spread_us=round(spread, 2), kv_bytes=nbytes, tbps=round(nbytes / t / 1e6, 3),
                       frac=round(nbytes / (t * 1e-6) / READ_CEILING, 3), copies=copies, reps=reps)
            rec.update(dict(kernel=bf16_kernel) if arm == "bf16" else
                       dict(n_splits=plan.n_splits, waves=plan.waves, kv_heads_per_wave=plan.kv_heads_per_wave,
                            heads_per_lane=plan.heads_per_lane, n_chunks=plan.n_chunks, grid=plan.grid))
            emit(rec)
        del c16, c8


def run_append(reps, emit):
    import torch
    from scalellm_amd import kernels
    from scalellm_amd.layers import HipAttnHandler
    dev, dt, H, KVH, n_slots, calls = "cuda", torch.bfloat16, 32, 8, 1 << 16, 16
    gen = torch.Generator(device=dev).manual_seed(2)
    inv_freq = 1.0 / (500000.0 ** (torch.arange(0, D, 2, dtype=torch.float32, device=dev) / D))
    cos_sin = HipAttnHandler.build_cos_sin(D, 8192, inv_freq)
    kc16, kc8 = torch.empty(n_slots, KVH, D, dtype=dt, device=dev), torch.empty(n_slots, KVH, D, dtype=torch.uint8, device=dev)
    vc16, vc8 = torch.empty_like(kc16), torch.empty_like(kc8)
    ks, vs = torch.full((KVH,), 0.02, device=dev), torch.full((KVH,), 0.03, device=dev)
    for T in (1, 32, 256):
        qkv = torch.randn(T, (H + 2 * KVH) * D, device=dev, generator=gen).to(dt)
        q, k, v = (qkv[:, a * D:b * D].view(T, -1, D) for a, b in ((0, H), (H, H + KVH), (H + KVH, H + 2 * KVH)))
        pos = torch.randint(0, 8192, (T,), device=dev, generator=gen).int()
        slots = torch.randperm(n_slots, device=dev, generator=gen)[:T].int()

        def fused():
            for _ in range(calls):
                kernels.apply_rotary_pos_emb(q, k, pos, cos_sin, D, False, value=v, slot_ids=slots, key_cache=kc16,
                                             value_cache=vc16)

        def pair():
            for _ in range(calls):
                kernels.apply_rotary_pos_emb(q, k, pos, cos_sin, D, False)
                kernels.set_kv_cache_fp8(slots, k, v, kc8, vc8, ks, vs)
        us = _time_arms({"fused_bf16": [_capture(fused) for _ in range(3)], "rope_then_fp8_append": [_capture(pair) for _ in range(3)]},
                        reps, calls)
        for arm, (t, spread) in us.items():
            emit(dict(kind="append", T=T, heads=H, kv_heads=KVH, head_dim=D, arm=arm, us=round(t, 2),
                      spread_us=round(spread, 2), reps=reps))


def run_step(reps, emit):
    import torch
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape, make_decode_inputs
    dev, bs_max = "cuda", 128
    shape = LlamaShape(n_layers=8)
    n_blocks = bs_max * (KV // BLOCK + 1) + 2
    os.environ["SLM_DECODE_LANES"] = "0"   # both arms on one lane: the fp8 cache has no two-lane form
    models = {name: LlamaDecodeStep(shape, bs_max, n_blocks, BLOCK, quant_method="awq", dtype=torch.bfloat16,
                                    device=dev, seed=0, kv_fill="tile", kv_cache_dtype=name) for name in ("auto", "fp8")}
    for bs in (1, 32, 128):
        tokens, positions, params, _ = make_decode_inputs(bs, KV, BLOCK, dev, seed=3, vocab=shape.vocab)
        arms = {}
        for name, m in models.items():
            m.reserve_workspaces(bs, KV)
            arms[name] = [_capture(lambda m=m: m.forward(tokens, positions, params)) for _ in range(3)]
        for name, (t, spread) in _time_arms(arms, reps, 1).items():
            emit(dict(kind="step", model="llama3_8b_awq_8_of_32_layers", bs=bs, kv_len=KV, kv_cache_dtype=name,
                      lanes=models[name].last_lanes, ms_per_step=round(t / 1e3, 3), spread_ms=round(spread / 1e3, 3), reps=reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_attn_fp8.jsonl"))
    ap.add_argument("--sections", default="attn,append,step")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--limit", type=int, default=400, help="seconds per section (child process)")
    ap.add_argument("--section", default=None, help=argparse.SUPPRESS)   # child mode
    args = ap.parse_args()
    if args.section is None:
        open(args.out, "w").close()
        for sec in args.sections.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--section", sec, "--out", args.out, "--reps", str(args.reps)]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"[bench_attn_fp8] section {sec} ended with {rc}: nothing more is started", file=sys.stderr)
                sys.exit(rc if rc > 0 else 1)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_attn_fp8 needs a GPU: there is no CPU fallback")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    {"attn": run_attn, "append": run_append, "step": run_step}[args.section](args.reps, emit)


if __name__ == "__main__":
    main()
