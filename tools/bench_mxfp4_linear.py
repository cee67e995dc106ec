#!/usr/bin/env python3
"""The MXFP4 weight-only linear, slm_mxfp4_linear, against the fp8 kernel, the dense kernel and the library GEMM on the
Llama-3-8B shapes.

    python tools/bench_mxfp4_linear.py [--out profiles/r22_mxfp4_linear.jsonl] [--ms 1,32,64,128] [--reps 15]

One JSON line per cell.  Per projection (qkv, o, gate_up plain and with the SiLU epilogue, down) and per M, bf16, four
columns timed in one session:

  mx_a/b/c     kernels.mxfp4_linear on the packed e2m1 weight and its e8m0 block scales (17/32 byte per weight)
  fp8_a/b/c    kernels.fp8_linear on a per-channel e4m3 quantisation of the dequantised weight (1 byte per weight)
  dense_a/b/c  kernels.linear on the dequantised bf16 weight (2 bytes per weight)
  lib_a/b/c    torch.nn.functional.linear on the same bf16 weight (gate_up + SiLU: then F.silu(gate) * up)

Every arm is a captured graph of one call per weight copy (the weights ROTATE over enough copies to exceed the
256 MiB last-level cache), replayed --reps times after a warm-up, the arms interleaved replay by replay; us = the
median replay over the copies.  The three repeats of an arm give its run-to-run spread: a row counts as faster only
when the slowest mxfp4 repeat beats the fastest repeat of the other column.  weight_gbps = weight bytes (nibbles +
scale bytes for mxfp4) / time, frac = that over the 7.0 TB/s read ceiling of profiles/r03_clock_under_load.jsonl.
"step": the 8-of-32-layer Llama-3-8B step at 4 k context, bs 1 and 32, quant_method "mxfp4" against "fp8" and "none",
interleaved in one process.

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

ARMS = ("mx_", "fp8_", "dense_", "lib_")


def run_shape(name, ms, reps, emit):
    import torch
    import torch.nn.functional as F
    from scalellm_amd import kernels
    K, N, silu = SHAPES[name]
    dev, dt = "cuda", torch.bfloat16
    bytes_per = {"mx_": K * N // 2 + K * N // 32, "fp8_": K * N, "dense_": 2 * K * N, "lib_": 2 * K * N}
    copies = {arm: max(2, -(-ROTATE_BYTES // b)) for arm, b in bytes_per.items()}
    gen = torch.Generator(device=dev).manual_seed(1)
    q4 = [kernels.quantize_mxfp4_weight(torch.randn(N, K, device=dev, generator=gen) * 0.02) for _ in range(copies["mx_"])]
    wd = [kernels.dequantize_mxfp4_weight(w, s, dt) for w, s in q4[:copies["dense_"]]]   # the load-time dequantisation
    q8 = [kernels.quantize_fp8_weight(kernels.dequantize_mxfp4_weight(w, s, dt)) for w, s in q4[:copies["fp8_"]]]
    n_out = N // 2 if silu else N
    for M in ms:
        a = torch.randn(M, K, device=dev, generator=gen).to(dt)
        c = torch.empty(M, n_out, dtype=dt, device=dev)

        def mx():
            for w, s in q4:
                kernels.mxfp4_linear(a, w, s, c, silu_mul=silu)

        def fp8():
            for w8, sc in q8:
                kernels.fp8_linear(a, w8, sc, c, silu_mul=silu)

        def dense():
            for w in wd:
                kernels.linear(a, w, c, silu_mul=silu)

        def lib():
            for w in wd:
                y = F.linear(a, w)
                if silu:
                    y = F.silu(y[:, :n_out]) * y[:, n_out:]
        info = kernels.mxfp4_linear_plan(a, q4[0][0], q4[0][1], c, silu_mul=silu)
        arms, calls = {}, {}
        for tag in "abc":
            for arm, fn in (("mx_", mx), ("fp8_", fp8), ("dense_", dense), ("lib_", lib)):
                arms[arm + tag], calls[arm + tag] = _capture(fn), copies[arm]
        us = {n: t * copies["mx_"] / calls[n] for n, t in _time_arms(arms, reps, copies["mx_"]).items()}   # per call
        rep = {k: [us[k + t] for t in "abc"] for k in ARMS}
        for arm, t in us.items():
            wbytes = bytes_per[arm[:-1]]
            rec = dict(kind="gemm", shape=name, M=M, K=K, N=N, arm=arm, us=round(t, 2), weight_bytes=wbytes,
                       weight_gbps=round(wbytes / t / 1e3, 1), frac=round(wbytes / (t * 1e-6) / READ_CEILING, 3),
                       copies=calls[arm], reps=reps)
            if arm == "mx_a":
                rec.update(row_tiles=info.row_tiles, waves=info.waves, split_k=info.split_k)
                for k in ARMS:
                    rec[k + "median_us"] = round(_median(rep[k]), 2)
                    rec[k + "spread_us"] = round(max(rep[k]) - min(rep[k]), 2)
                for k in ARMS[1:]:
                    rec["faster_than_" + k[:-1]] = bool(max(rep["mx_"]) < min(rep[k]))
            emit(rec)
        del arms


def run_step(reps, emit):
    import torch
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape, make_decode_inputs
    dev, B, kv = "cuda", 16, 4096
    shape = LlamaShape(n_layers=8)
    n_blocks = 32 * (kv // B + 1) + 2
    models = {q: LlamaDecodeStep(shape, 32, n_blocks, B, quant_method=q, dtype=torch.bfloat16, device=dev, seed=0,
                                 kv_fill="tile") for q in ("none", "fp8", "mxfp4")}
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
                      layer_weight_bytes=int(elems * model.weight_bits) // 8, reps=reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_mxfp4_linear.jsonl"))
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
                print(f"[bench_mxfp4_linear] section {sec} ended with {rc}: nothing more is started", file=sys.stderr)
                sys.exit(rc if rc > 0 else 1)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mxfp4_linear needs a GPU: there is no CPU fallback")

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
