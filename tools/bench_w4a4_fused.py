#!/usr/bin/env python3
"""The MXFP4 quantiser in the producers (include/slm_hip.h section 24) against the launches it replaces, bf16.

    python tools/bench_w4a4_fused.py [--out profiles/r26_w4a4_fused.jsonl] [--ms 1,32,64,128] [--reps 15]

One JSON line per cell; every cell holds the median of three interleaved repeats per arm and their spread.

  "norm"   hidden 4096, T = 1 / 32 / 256, forms plain / residual / 4 split-K slabs: kernels.rms_norm_mxfp4 (fused)
           against the captured pair rms_norm + quantize_mxfp4_act (pair) and against rms_norm alone (norm)
  "gemm"   Llama-3-8B shapes: qkv and down on the pre-quantised side (q) against their T side (t); gate_up with the
           SiLU epilogue: T in / T out (t_t, the unfused step's call), T in / MXFP4 out (t_q: the epilogue alone) and
           pre-quantised in / MXFP4 out (q_q, the fused step's call)
  "step"   the 8-of-32-layer Llama-3-8B step at 4 k context, bs 1 and 32: W4A4 with fuse_act_quant (fused) against
           W4A4 without (unfused) and against W4A16 (w4a16), interleaved in one process

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
from bench_w4a4_linear import _verdict  # noqa: E402

NORM_CALLS = 40   # norm launches per graph: a replay is long against the event resolution


def _cells(arms_fns, reps, calls, first):
    """arms_fns: name -> fn; three captured repeats per arm, interleaved.  Returns the record fields."""
    arms = {f"{n}_{t}": _capture(fn) for t in "abc" for n, fn in arms_fns.items()}
    us = _time_arms(arms, reps, calls)
    rep = {n: [us[f"{n}_{t}"] for t in "abc"] for n in arms_fns}
    rec = {}
    for n in arms_fns:
        rec[n + "_median_us"], rec[n + "_spread_us"] = round(_median(rep[n]), 2), round(max(rep[n]) - min(rep[n]), 2)
        if n != first:
            rec[f"{first}_vs_{n}"] = _verdict(rep[first], rep[n])
    return rec


def run_norm(reps, emit):
    import torch
    from scalellm_amd import kernels
    dev, dt, H, eps = "cuda", torch.bfloat16, 4096, 1e-5
    gen = torch.Generator(device=dev).manual_seed(1)
    weight = (1 + 0.05 * torch.randn(H, device=dev, generator=gen)).to(dt)
    wq, ws = kernels.quantize_mxfp4_weight(torch.randn(H, H, device=dev, generator=gen) * 0.02)
    for T in (1, 32, 256):
        x = torch.randn(T, H, device=dev, generator=gen).to(dt)
        out, aq, asc = torch.empty_like(x), torch.empty(T, H // 2, dtype=torch.uint8, device=dev), \
            torch.empty(T, H // 32, dtype=torch.uint8, device=dev)
        for form in ("plain", "residual", "slabs4"):
            res = torch.zeros_like(x) if form != "plain" else None     # (x is added to it launch by launch: stays finite)
            with kernels.tuning(SLM_W4A4_SPLITK=4):
                h = kernels.w4a4_linear(x, wq, ws, out, defer_reduce=True) if form == "slabs4" else None
            assert form != "slabs4" or int(h) == 4
            kw = dict(residual=res, partials=h)

            def fused():
                for _ in range(NORM_CALLS):
                    kernels.rms_norm_mxfp4(x, weight, eps, aq=aq, a_scale=asc, **kw)

            def pair():
                for _ in range(NORM_CALLS):
                    kernels.rms_norm(out, x, weight, eps, **kw)
                    kernels.quantize_mxfp4_act(out, aq, asc)

            def norm():
                for _ in range(NORM_CALLS):
                    kernels.rms_norm(out, x, weight, eps, **kw)
            emit(dict(kind="norm", T=T, hidden=H, form=form, reps=reps,
                      **_cells(dict(fused=fused, pair=pair, norm=norm), reps, NORM_CALLS, "fused")))


def run_shape(name, ms, reps, emit):
    import torch
    from scalellm_amd import kernels
    K, N, silu = SHAPES[name]
    dev, dt = "cuda", torch.bfloat16
    copies = max(2, -(-ROTATE_BYTES // (K * N // 2 + K * N // 32)))
    gen = torch.Generator(device=dev).manual_seed(1)
    q4 = [kernels.quantize_mxfp4_weight(torch.randn(N, K, device=dev, generator=gen) * 0.02) for _ in range(copies)]
    for M in ms:
        a = torch.randn(M, K, device=dev, generator=gen).to(dt)
        aq, asc = kernels.quantize_mxfp4_act(a)
        c = torch.empty(M, N // 2 if silu else N, dtype=dt, device=dev)
        cq, cs = torch.empty(M, N // 4, dtype=torch.uint8, device=dev), torch.empty(M, N // 64, dtype=torch.uint8, device=dev)

        def arm(a_in, a_scale, quant_out):
            def fn():
                for w, s in q4:
                    if quant_out:
                        kernels.w4a4_linear(a_in, w, s, cq, silu_mul=True, a_scale=a_scale, c_scale=cs, dtype=dt)
                    else:
                        kernels.w4a4_linear(a_in, w, s, c, silu_mul=silu, a_scale=a_scale)
            return fn
        if silu:
            fns, first = dict(q_q=arm(aq, asc, True), t_q=arm(a, None, True), t_t=arm(a, None, False)), "q_q"
        else:
            fns, first = dict(q=arm(aq, asc, False), t=arm(a, None, False)), "q"
        info = kernels.w4a4_linear_plan(a, q4[0][0], q4[0][1], c, silu_mul=silu)
        emit(dict(kind="gemm", shape=name, M=M, K=K, N=N, row_tiles=info.row_tiles, waves=info.waves,
                  split_k=info.split_k, copies=copies, reps=reps, **_cells(fns, reps, copies, first)))


def run_step(reps, emit):
    import torch
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape, make_decode_inputs
    dev, B, kv = "cuda", 16, 4096
    shape = LlamaShape(n_layers=8)
    n_blocks = 32 * (kv // B + 1) + 2
    kinds = {"fused": dict(act_quant="mxfp4", fuse_act_quant=True), "unfused": dict(act_quant="mxfp4"), "w4a16": dict()}
    models = {n: LlamaDecodeStep(shape, 32, n_blocks, B, dtype=torch.bfloat16, device=dev, seed=0, kv_fill="tile",
                                 quant_method="mxfp4", **kw) for n, kw in kinds.items()}
    for bs in (1, 32):
        tokens, positions, params, _ = make_decode_inputs(bs, kv, B, dev, seed=3, vocab=shape.vocab)
        fns = {}
        for q, model in models.items():
            model.reserve_workspaces(bs, kv)
            fns[q] = lambda model=model: model.forward(tokens, positions, params)
        same = bool(torch.equal(fns["fused"](), fns["unfused"]()))     # the same next tokens before anything is timed
        emit(dict(kind="step", model="llama3_8b_mxfp4_bf16_8_of_32_layers", bs=bs, kv_len=kv, reps=reps,
                  fused_equals_unfused=same, **_cells(fns, reps, 1, "fused")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_w4a4_fused.jsonl"))
    ap.add_argument("--ms", default="1,32,64,128")
    ap.add_argument("--shapes", default="qkv,down,gate_up_silu")
    ap.add_argument("--sections", default="norm,gemm,step")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--limit", type=int, default=300, help="seconds per section (child process)")
    ap.add_argument("--section", default=None, help=argparse.SUPPRESS)   # child mode
    args = ap.parse_args()
    if args.section is None:
        want = args.sections.split(",")
        secs = (["norm"] if "norm" in want else []) + \
            (["gemm:" + s for s in args.shapes.split(",")] if "gemm" in want else []) + (["step"] if "step" in want else [])
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
                print(f"[bench_w4a4_fused] section {sec} ended with {rc}: nothing more is started", file=sys.stderr)
                sys.exit(rc if rc > 0 else 1)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_w4a4_fused needs a GPU: there is no CPU fallback")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if args.section == "norm":
        run_norm(args.reps, emit)
    elif args.section.startswith("gemm:"):
        run_shape(args.section[5:], [int(x) for x in args.ms.split(",")], args.reps, emit)
    else:
        run_step(args.reps, emit)


if __name__ == "__main__":
    main()
