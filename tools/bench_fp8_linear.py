#!/usr/bin/env python3
"""The fp8 (e4m3) weight-only linear, slm_fp8_linear, against the dense kernel and the library GEMM on the Llama-3-8B
shapes.

    python tools/bench_fp8_linear.py [--out profiles/r17_fp8_linear.jsonl] [--ms 1,32,64,128] [--reps 15]

One JSON line per cell.  Per projection (qkv, o, gate_up plain and with the SiLU epilogue, down) and per M, bf16:

  fp8_a/b/c    kernels.fp8_linear on the e4m3 weight and its per-channel scale
  dense_a/b/c  kernels.linear on T(W8), the same codes converted to bf16 (twice the weight bytes)
  lib_a/b/c    torch.nn.functional.linear on the dequantised bf16 weight (gate_up + SiLU: then F.silu(gate) * up)

Every arm is a captured graph of one call per weight copy (the weights ROTATE over enough copies to exceed the
256 MiB last-level cache), replayed --reps times after a warm-up, the arms interleaved replay by replay; us = the
median replay over the copies.  The three repeats of an arm give its run-to-run spread: a row counts as faster only
when the slowest fp8 repeat beats the fastest dense repeat.  weight_gbps = weight bytes / time, frac = that over the
7.0 TB/s read ceiling of profiles/r03_clock_under_load.jsonl.  "step": the 8-of-32-layer Llama-3-8B step at 4 k
context, bs 1 and 32, quant_method "fp8" against "none", interleaved in one process.

Every section runs in a child process of its own under a time limit (--limit seconds); the first section that fails
or overruns ends the run, nothing more is started."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_dense_gemm import READ_CEILING, ROTATE_BYTES, SHAPES, _capture, _median, _time_arms  # noqa: E402


def run_shape(name, ms, reps, emit):
    import torch
    import torch.nn.functional as F
    from scalellm_amd import kernels
    K, N, silu = SHAPES[name]
    dev, dt = "cuda", torch.bfloat16
    copies8 = max(2, -(-ROTATE_BYTES // (K * N)))
    copies16 = max(2, -(-ROTATE_BYTES // (2 * K * N)))
    gen = torch.Generator(device=dev).manual_seed(1)
    q8 = [kernels.quantize_fp8_weight(torch.randn(N, K, device=dev, generator=gen) * 0.02) for _ in range(copies8)]
    wt = [w8.to(dt) for w8, _ in q8[:copies16]]                        # T(W8): what the dense kernel streams
    wd = [(w8.float() * sc[:, None]).to(dt) for w8, sc in q8[:copies16]]   # the load-time dequantisation
    n_out = N // 2 if silu else N
    for M in ms:
        a = torch.randn(M, K, device=dev, generator=gen).to(dt)
        c = torch.empty(M, n_out, dtype=dt, device=dev)

        def fp8():
            for w8, sc in q8:
                kernels.fp8_linear(a, w8, sc, c, silu_mul=silu)

        def dense():
            for w in wt:
                kernels.linear(a, w, c, silu_mul=silu)

        def lib():
            for w in wd:
                y = F.linear(a, w)
                if silu:
                    y = F.silu(y[:, :n_out]) * y[:, n_out:]
        info = kernels.fp8_linear_plan(a, q8[0][0], q8[0][1], c, silu_mul=silu)
        arms, calls = {}, {}
        for tag in "abc":
            for arm, fn, n in (("fp8_", fp8, copies8), ("dense_", dense, copies16), ("lib_", lib, copies16)):
                arms[arm + tag], calls[arm + tag] = _capture(fn), n
        us = {n: t * copies8 / calls[n] for n, t in _time_arms(arms, reps, copies8).items()}   # per call of the arm
        rep = {k: [us[k + t] for t in "abc"] for k in ("fp8_", "dense_", "lib_")}
        for arm, t in us.items():
            wbytes = K * N * (1 if arm.startswith("fp8") else 2)
            rec = dict(kind="gemm", shape=name, M=M, K=K, N=N, arm=arm, us=round(t, 2), weight_bytes=wbytes,
                       weight_gbps=round(wbytes / t / 1e3, 1), frac=round(wbytes / (t * 1e-6) / READ_CEILING, 3),
                       copies=calls[arm], reps=reps)
            if arm == "fp8_a":
                rec.update(row_tiles=info.row_tiles, waves=info.waves, split_k=info.split_k,
                           fp8_median_us=round(_median(rep["fp8_"]), 2),
                           fp8_spread_us=round(max(rep["fp8_"]) - min(rep["fp8_"]), 2),
                           dense_median_us=round(_median(rep["dense_"]), 2),
                           dense_spread_us=round(max(rep["dense_"]) - min(rep["dense_"]), 2),
                           lib_median_us=round(_median(rep["lib_"]), 2),
                           lib_spread_us=round(max(rep["lib_"]) - min(rep["lib_"]), 2),
                           faster_than_dense=bool(max(rep["fp8_"]) < min(rep["dense_"])))
            emit(rec)
        del arms


def run_step(reps, emit):
    import torch
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape, make_decode_inputs
    dev, B, kv = "cuda", 16, 4096
    shape = LlamaShape(n_layers=8)
    n_blocks = 32 * (kv // B + 1) + 2
    models = {q: LlamaDecodeStep(shape, 32, n_blocks, B, quant_method=q, dtype=torch.bfloat16, device=dev, seed=0,
                                 kv_fill="tile") for q in ("none", "fp8")}
    elems = 4096 * 6144 + 4096 * 4096 + 3 * 4096 * 14336
    for bs in (1, 32):
        tokens, positions, params, _ = make_decode_inputs(bs, kv, B, dev, seed=3, vocab=shape.vocab)
        arms = {}
        for q, model in models.items():
            model.reserve_workspaces(bs, kv)
            for tag in "abc":
                arms[f"{q}_{tag}"] = _capture(lambda model=model: model.forward(tokens, positions, params))
        us = _time_arms(arms, reps, 1)
        for q, model in models.items():
            ts = [us[f"{q}_{t}"] for t in "abc"]
            emit(dict(kind="step", model=f"llama3_8b_{q}_bf16_8_of_32_layers", quant_method=q, bs=bs, kv_len=kv,
                      lanes=model.last_lanes, ms_per_step=round(_median(ts) / 1e3, 3),
                      spread_ms=round((max(ts) - min(ts)) / 1e3, 3),
                      layer_weight_bytes=elems * (1 if q == "fp8" else 2), reps=reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_fp8_linear.jsonl"))
    ap.add_argument("--ms", default="1,32,64,128")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--sections", default="gemm,step")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--limit", type=int, default=300, help="seconds per section (child process)")
    ap.add_argument("--section", default=None, help=argparse.SUPPRESS)   # child mode
    args = ap.parse_args()
    ms = [int(x) for x in args.ms.split(",")]
    if args.section is None:
        want = args.sections.split(",")
        secs = (["gemm:" + s for s in args.shapes.split(",")] if "gemm" in want else []) + \
            (["step"] if "step" in want else [])
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
                print(f"[bench_fp8_linear] section {sec} ended with {rc}: nothing more is started", file=sys.stderr)
                sys.exit(rc if rc > 0 else 1)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_fp8_linear needs a GPU: there is no CPU fallback")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if args.section.startswith("gemm:"):
        run_shape(args.section[5:], ms, args.reps, emit)
    else:
        run_step(args.reps, emit)


if __name__ == "__main__":
    main()
