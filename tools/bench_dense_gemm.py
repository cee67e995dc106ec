#!/usr/bin/env python3
"""The dense (unquantised bf16) linear, slm_linear, against the library GEMM on the Llama-3-8B shapes.

    python tools/bench_dense_gemm.py [--out profiles/r14_dense.jsonl] [--ms 1,4,8,16,32,64,128,256] [--reps 15]

One JSON line per cell.  Per projection (qkv 4096 -> 6144, o 4096 -> 4096, gate_up 4096 -> 28672 plain and with the
SiLU epilogue, down 14336 -> 4096) and per M:

  native     kernels.linear with the plan's own K split
  unsplit    the same under SLM_LINEAR_SPLITK=1 (o and down at M <= 32: the shapes the K split exists for)
  lib_a/b/c  torch.nn.functional.linear on the same tensors (the library GEMM), three times: their spread is what
             counts as a difference; gate_up + SiLU: F.linear then F.silu(gate) * up

Every arm is a captured graph of one call per weight copy (the weights ROTATE over enough copies to exceed the
256 MiB last-level cache), replayed --reps times after a warm-up, the arms interleaved replay by replay; us = the
median replay over the copies.  weight_gbps = weight bytes / time, frac = that over the 7.0 TB/s read ceiling of
profiles/r03_clock_under_load.jsonl.  "chain": one decoder layer's four GEMMs with their glue (deferred slabs into
rms_norm, SiLU epilogue) against the library chain with torch add / norm.  "step": a dense 8-of-32-layer Llama-3-8B
step at 4 k context, bs 1 and 32.

Every section runs in a child process of its own under a time limit (--limit seconds); the first section that fails
or overruns ends the run, nothing more is started."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ_CEILING = 7.0e12   # bytes / s, profiles/r03_clock_under_load.jsonl
SHAPES = {"qkv": (4096, 6144, False), "o": (4096, 4096, False), "gate_up": (4096, 28672, False),
          "gate_up_silu": (4096, 28672, True), "down": (14336, 4096, False)}   # K, N, silu
ROTATE_BYTES = 640 << 20


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def _time_arms(arms, reps, calls):
    """arms: name -> captured graph of `calls` calls; interleaved replays, median us per call"""
    import torch
    for g in arms.values():
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    times = {n: [] for n in arms}
    for _ in range(reps):
        for n, g in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / calls)
    return {n: _median(t) for n, t in times.items()}


def _capture(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def run_shape(name, ms, reps, emit):
    import torch
    import torch.nn.functional as F
    from scalellm_amd import kernels
    K, N, silu = SHAPES[name]
    dev, dt = "cuda", torch.bfloat16
    wbytes = K * N * 2
    copies = max(2, -(-ROTATE_BYTES // wbytes))
    gen = torch.Generator(device=dev).manual_seed(1)
    ws = [(torch.randn(N, K, device=dev, generator=gen) * 0.02).to(dt) for _ in range(copies)]
    n_out = N // 2 if silu else N
    for M in ms:
        a = torch.randn(M, K, device=dev, generator=gen).to(dt)
        c = torch.empty(M, n_out, dtype=dt, device=dev)

        def native():
            for w in ws:
                kernels.linear(a, w, c, silu_mul=silu)

        def lib():
            for w in ws:
                y = F.linear(a, w)
                if silu:
                    y = F.silu(y[:, :n_out]) * y[:, n_out:]
        info = kernels.linear_plan(a, ws[0], c, silu_mul=silu)
        arms = {"native": _capture(native)}
        if name in ("o", "down") and M <= 32:
            with kernels.tuning(SLM_LINEAR_SPLITK=1):
                arms["unsplit"] = _capture(native)
        for tag in "abc":
            arms["lib_" + tag] = _capture(lib)
        us = _time_arms(arms, reps, copies)
        libs = [us["lib_a"], us["lib_b"], us["lib_c"]]
        for arm, t in us.items():
            rec = dict(kind="gemm", shape=name, M=M, K=K, N=N, arm=arm, us=round(t, 2), weight_bytes=wbytes,
                       weight_gbps=round(wbytes / t / 1e3, 1), frac=round(wbytes / (t * 1e-6) / READ_CEILING, 3),
                       copies=copies, reps=reps)
            if arm in ("native", "unsplit"):
                rec.update(row_tiles=info.row_tiles, waves=info.waves, split_k=1 if arm == "unsplit" else info.split_k,
                           lib_median_us=round(_median(libs), 2), lib_spread_us=round(max(libs) - min(libs), 2))
            emit(rec)
        del arms


def run_chain(ms, reps, emit):
    """one decoder layer's GEMMs and glue (no attention: the o projection reads the q columns of the qkv output)"""
    import torch
    import torch.nn.functional as F
    from scalellm_amd import kernels
    dev, dt, H, I, QKV = "cuda", torch.bfloat16, 4096, 14336, 6144
    gen = torch.Generator(device=dev).manual_seed(2)
    layer_bytes = 2 * (H * QKV + H * H + 3 * H * I)
    copies = max(2, -(-ROTATE_BYTES // layer_bytes))
    mk = lambda n, k: (torch.randn(n, k, device=dev, generator=gen) * 0.02).to(dt)  # noqa: E731
    Ls = [dict(qkv=mk(QKV, H), o=mk(H, H), gu=mk(2 * I, H), down=mk(H, I)) for _ in range(copies)]
    nw_ = torch.ones(H, dtype=dt, device=dev)
    for M in ms:
        normed = torch.randn(M, H, device=dev, generator=gen).to(dt)
        resid = torch.zeros(M, H, dtype=dt, device=dev)
        qkv, o, act, down = (torch.empty(M, n, dtype=dt, device=dev) for n in (QKV, H, I, H))
        nrm = torch.empty(M, H, dtype=dt, device=dev)

        def native():
            for L in Ls:
                kernels.linear(normed, L["qkv"], qkv)
                h = kernels.linear(qkv[:, :H], L["o"], o, defer_reduce=True)
                kernels.rms_norm(nrm, o, nw_, 1e-5, residual=resid, partials=h)
                kernels.linear(nrm, L["gu"], act, silu_mul=True)
                h = kernels.linear(act, L["down"], down, defer_reduce=True)
                kernels.rms_norm(nrm, down, nw_, 1e-5, residual=resid, partials=h)

        def norm(x):
            xf = x.float()
            return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).to(dt) * nw_

        def lib():
            r = resid
            for L in Ls:
                y = F.linear(normed, L["qkv"])
                r = r + F.linear(y[:, :H], L["o"])
                n1 = norm(r)
                gu = F.linear(n1, L["gu"])
                r = r + F.linear(F.silu(gu[:, :I]) * gu[:, I:], L["down"])
                norm(r)
        arms = {"native": _capture(native)}
        for tag in "abc":
            arms["lib_" + tag] = _capture(lib)
        us = _time_arms(arms, reps, copies)
        libs = [us["lib_a"], us["lib_b"], us["lib_c"]]
        for arm, t in us.items():
            rec = dict(kind="chain", M=M, arm=arm, us=round(t, 2), weight_bytes=layer_bytes,
                       weight_gbps=round(layer_bytes / t / 1e3, 1), frac=round(layer_bytes / (t * 1e-6) / READ_CEILING, 3),
                       copies=copies, reps=reps)
            if arm == "native":
                rec.update(lib_median_us=round(_median(libs), 2), lib_spread_us=round(max(libs) - min(libs), 2))
            emit(rec)
        del arms


def run_step(reps, emit):
    import torch
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape, make_decode_inputs
    dev, B, kv = "cuda", 16, 4096
    shape = LlamaShape(n_layers=8)
    n_blocks = 32 * (kv // B + 1) + 2
    model = LlamaDecodeStep(shape, 32, n_blocks, B, quant_method="none", dtype=torch.bfloat16, device=dev, seed=0,
                            kv_fill="tile")
    for bs in (1, 32):
        tokens, positions, params, _ = make_decode_inputs(bs, kv, B, dev, seed=3, vocab=shape.vocab)
        model.reserve_workspaces(bs, kv)
        g = _capture(lambda: model.forward(tokens, positions, params))
        t = _time_arms({"step": g}, reps, 1)["step"]
        layer_bytes = 2 * (4096 * 6144 + 4096 * 4096 + 3 * 4096 * 14336)
        emit(dict(kind="step", model="llama3_8b_dense_bf16_8_of_32_layers", bs=bs, kv_len=kv, lanes=model.last_lanes,
                  ms_per_step=round(t / 1e3, 3), layer_weight_bytes=layer_bytes, reps=reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_dense.jsonl"))
    ap.add_argument("--ms", default="1,4,8,16,32,64,128,256")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--sections", default="gemm,chain,step")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--limit", type=int, default=300, help="seconds per section (child process)")
    ap.add_argument("--section", default=None, help=argparse.SUPPRESS)   # child mode
    args = ap.parse_args()
    ms = [int(x) for x in args.ms.split(",")]
    if args.section is None:
        secs = []
        want = args.sections.split(",")
        if "gemm" in want:
            secs += ["gemm:" + s for s in args.shapes.split(",")]
        secs += [s for s in ("chain", "step") if s in want]
        open(args.out, "w").close()
        for sec in secs:
            cmd = [sys.executable, os.path.abspath(__file__), "--section", sec, "--out", args.out, "--ms", args.ms,
                   "--reps", str(args.reps)]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"[bench_dense_gemm] section {sec} ended with {rc}: nothing more is started", file=sys.stderr)
                sys.exit(rc if rc > 0 else 1)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_dense_gemm needs a GPU: there is no CPU fallback")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if args.section.startswith("gemm:"):
        run_shape(args.section[5:], ms, args.reps, emit)
    elif args.section == "chain":
        run_chain([m for m in ms if m in (1, 32, 128)] or ms[:1], args.reps, emit)
    else:
        run_step(args.reps, emit)


if __name__ == "__main__":
    main()
