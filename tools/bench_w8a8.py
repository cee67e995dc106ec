#!/usr/bin/env python3
"""The fp8 x fp8 linear (include/slm_hip.h section 25) against the fp8 weight-only linear and torch, bf16.

    python tools/bench_w8a8.py [--out profiles/r27_w8a8_linear.jsonl] [--ms 1,32,64,128,256] [--reps 15]

One JSON line per cell; every cell holds the median of three interleaved repeats per arm and their spread.

  "gemm"   Llama-3-8B shapes qkv / o / gate_up / gate_up + SiLU / down: kernels.w8a8_linear on pre-quantised input
           (w8a8), quantize_fp8_act + w8a8_linear (q_w8a8: what a layer with act_quant="fp8" launches),
           kernels.fp8_linear (fp8: W8A16) and F.linear on the dequantised bf16 weight (torch)
  "quant"  kernels.quantize_fp8_act alone, hidden 4096 and 14336, T = 1 / 32 / 256
  "step"   the 8-of-32-layer Llama-3-8B step at 4 k context, bs 1 / 32 / 128: act_quant="fp8" (w8a8) against
           act_quant=None (w8a16), interleaved in one process

Method as tools/bench_w4a4_linear.py: captured graphs, the GEMM weights ROTATE over enough copies to exceed the
last-level cache, arms interleaved replay by replay; a row counts as faster only when the slowest repeat of the first
arm beats the fastest repeat of the other ("slower": the other way round; else "tie").  Every section runs in a child
process of its own under a time limit (--limit seconds); the first that fails or overruns ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_dense_gemm import ROTATE_BYTES, SHAPES, _capture, _median, _time_arms  # noqa: E402

QUANT_CALLS = 40   # quantiser launches per graph: a replay is long against the event resolution


def _verdict(ours, other):
    return "faster" if max(ours) < min(other) else "slower" if min(ours) > max(other) else "tie"


def _cells(arms_fns, reps, calls, pairs):
    """arms_fns: name -> fn; three captured repeats per arm, interleaved.  Returns the record fields: per arm the
    median and the spread of its repeats, per (a, b) of `pairs` the verdict a_vs_b."""
    arms = {f"{n}_{t}": _capture(fn) for t in "abc" for n, fn in arms_fns.items()}
    us = _time_arms(arms, reps, calls)
    rep = {n: [us[f"{n}_{t}"] for t in "abc"] for n in arms_fns}
    rec = {}
    for n in arms_fns:
        rec[n + "_median_us"], rec[n + "_spread_us"] = round(_median(rep[n]), 2), round(max(rep[n]) - min(rep[n]), 2)
    for a, b in pairs:
        rec[f"{a}_vs_{b}"] = _verdict(rep[a], rep[b])
    return rec


def run_shape(name, ms, reps, emit):
    import torch
    import torch.nn.functional as F
    from scalellm_amd import kernels
    K, N, silu = SHAPES[name]
    dev, dt = "cuda", torch.bfloat16
    copies = max(2, -(-ROTATE_BYTES // (K * N)))
    gen = torch.Generator(device=dev).manual_seed(1)
    q8 = [kernels.quantize_fp8_weight(torch.randn(N, K, device=dev, generator=gen) * 0.02) for _ in range(copies)]
    wt = [(w.to(dt) * s[:, None].to(dt)) for w, s in q8[:max(2, -(-ROTATE_BYTES // (2 * K * N)))]]
    n_out = N // 2 if silu else N
    for M in ms:
        a = torch.randn(M, K, device=dev, generator=gen).to(dt)
        aq, asc = kernels.quantize_fp8_act(a)
        c = torch.empty(M, n_out, dtype=dt, device=dev)

        def w8a8():
            for w, s in q8:
                kernels.w8a8_linear(aq, asc, w, s, c, silu_mul=silu)

        def q_w8a8():
            for w, s in q8:
                kernels.quantize_fp8_act(a, aq=aq, a_scale=asc)
                kernels.w8a8_linear(aq, asc, w, s, c, silu_mul=silu)

        def fp8():
            for w, s in q8:
                kernels.fp8_linear(a, w, s, c, silu_mul=silu)

        def lib():   # (as many calls, over fewer bf16 copies of twice the size: the same bytes between reuses)
            for i in range(copies):
                y = F.linear(a, wt[i % len(wt)])
                if silu:
                    y = F.silu(y[:, :n_out]) * y[:, n_out:]
        info = kernels.w8a8_linear_plan(aq, asc, q8[0][0], q8[0][1], c, silu_mul=silu)
        emit(dict(kind="gemm", shape=name, M=M, K=K, N=N, row_tiles=info.row_tiles, waves=info.waves,
                  split_k=info.split_k, copies=copies, reps=reps,
                  **_cells(dict(w8a8=w8a8, q_w8a8=q_w8a8, fp8=fp8, torch=lib), reps, copies,
                           (("w8a8", "fp8"), ("w8a8", "torch"), ("q_w8a8", "fp8"), ("q_w8a8", "torch")))))


def run_quant(reps, emit):
    import torch
    from scalellm_amd import kernels
    dev, dt = "cuda", torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(1)
    for H in (4096, 14336):
        for T in (1, 32, 256):
            x = torch.randn(T, H, device=dev, generator=gen).to(dt)
            aq, asc = kernels.quantize_fp8_act(x)
            st = torch.tensor([0.01], device=dev)

            def dynamic():
                for _ in range(QUANT_CALLS):
                    kernels.quantize_fp8_act(x, aq=aq, a_scale=asc)

            def static():
                for _ in range(QUANT_CALLS):
                    kernels.quantize_fp8_act(x, st, aq=aq, a_scale=asc)
            emit(dict(kind="quant", T=T, hidden=H, bytes=3 * T * H, reps=reps,
                      **_cells(dict(dynamic=dynamic, static=static), reps, QUANT_CALLS, (("dynamic", "static"),))))


def run_step(reps, emit):
    import torch
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape, make_decode_inputs
    dev, B, kv = "cuda", 16, 4096
    shape = LlamaShape(n_layers=8)
    n_blocks = 128 * (kv // B + 1) + 2
    models = {n: LlamaDecodeStep(shape, 128, n_blocks, B, dtype=torch.bfloat16, device=dev, seed=0, kv_fill="tile",
                                 quant_method="fp8", **kw) for n, kw in (("w8a8", dict(act_quant="fp8")), ("w8a16", dict()))}
    for bs in (1, 32, 128):
        tokens, positions, params, _ = make_decode_inputs(bs, kv, B, dev, seed=3, vocab=shape.vocab)
        fns = {}
        for q, model in models.items():
            model.reserve_workspaces(bs, kv)
            fns[q] = lambda model=model: model.forward(tokens, positions, params)
        agree = float((fns["w8a8"]() == fns["w8a16"]()).float().mean())   # the same next tokens, as a share
        emit(dict(kind="step", model="llama3_8b_fp8_bf16_8_of_32_layers", bs=bs, kv_len=kv, reps=reps,
                  next_tokens_agreeing=round(agree, 3), **_cells(fns, reps, 1, (("w8a8", "w8a16"),))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_w8a8_linear.jsonl"))
    ap.add_argument("--ms", default="1,32,64,128,256")
    ap.add_argument("--shapes", default="qkv,o,gate_up,gate_up_silu,down")
    ap.add_argument("--sections", default="gemm,quant,step")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--limit", type=int, default=300, help="seconds per section (child process)")
    ap.add_argument("--section", default=None, help=argparse.SUPPRESS)   # child mode
    args = ap.parse_args()
    if args.section is None:
        want = args.sections.split(",")
        secs = (["gemm:" + s for s in args.shapes.split(",")] if "gemm" in want else []) + \
            (["quant"] if "quant" in want else []) + (["step"] if "step" in want else [])
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()
        for sec in secs:
            cmd = [sys.executable, os.path.abspath(__file__), "--section", sec, "--out", args.out, "--ms", args.ms,
                   "--reps", str(args.reps)]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"[bench_w8a8] section {sec} ended with {rc}: nothing more is started", file=sys.stderr)
                sys.exit(rc if rc > 0 else 1)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_w8a8 needs a GPU: there is no CPU fallback")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if args.section.startswith("gemm:"):
        run_shape(args.section[5:], [int(x) for x in args.ms.split(",")], args.reps, emit)
    elif args.section == "quant":
        run_quant(args.reps, emit)
    else:
        run_step(args.reps, emit)


if __name__ == "__main__":
    main()
