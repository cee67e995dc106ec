#!/usr/bin/env python3
"""A/B of the ring depth of dense.hip's mxfp4 weight side (SLM_LIN_MX_RING).

    for r in 4 6 8; do tools/build_variant.sh mxring$r dense.hip -DSLM_LIN_MX_RING=$r; done
    python tools/ab_mxfp4_ring.py [--out profiles/r22_mxfp4_ring_ab.jsonl] [--rings 3,4,6,8,3]

One child process per library build -- ring 3 is the tree's libslm_hip.so, ring R tools/probes/tmp_libs/mxring<R>.so --
one after the other on one machine; the default order ends with the tree's build again, so the two ring-3 runs show
the drift between processes.  Per build: the mxfp4 arm of tools/bench_mxfp4_linear.py (graph replay over rotating
weight copies, three repeats interleaved) on gate_up, down, o and qkv at M 1 / 32 / 128.  One JSON line per repeat:
kind "ring_ab", the plan, `ring`, `us`, weight bytes over time, and `out_sha1`, the digest of the last output -- equal
across the builds of a row, since no result bit depends on the depth.  A child that fails or overruns ends the run."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def child(ring, lib, out):
    import torch
    from scalellm_amd import _lib
    if lib:
        _lib.LIB_PATH = lib                                  # before the first call loads the library
    from scalellm_amd import kernels
    from bench_dense_gemm import READ_CEILING, ROTATE_BYTES, SHAPES, _capture, _time_arms
    if not torch.cuda.is_available():
        sys.exit("ab_mxfp4_ring needs a GPU: there is no CPU fallback")
    dev, dt = "cuda", torch.bfloat16
    for name in ("gate_up", "down", "o", "qkv"):
        K, N, _ = SHAPES[name]
        wbytes = K * N // 2 + K * N // 32
        copies = max(2, -(-ROTATE_BYTES // wbytes))
        gen = torch.Generator(device=dev).manual_seed(1)
        q4 = [kernels.quantize_mxfp4_weight(torch.randn(N, K, device=dev, generator=gen) * 0.02) for _ in range(copies)]
        for M in (1, 32, 128):
            a = torch.randn(M, K, device=dev, generator=gen).to(dt)
            c = torch.empty(M, N, dtype=dt, device=dev)

            def mx():
                for w, s in q4:
                    kernels.mxfp4_linear(a, w, s, c)
            info = kernels.mxfp4_linear_plan(a, q4[0][0], q4[0][1], c)
            arms = {"mx_" + t: _capture(mx) for t in "abc"}
            us = _time_arms(arms, 15, copies)
            torch.cuda.synchronize()
            digest = hashlib.sha1(c.view(torch.int16).cpu().numpy().tobytes()).hexdigest()[:12]
            for arm, t in us.items():
                line = json.dumps(dict(
                    kind="ring_ab", shape=name, M=M, K=K, N=N, row_tiles=info.row_tiles, waves=info.waves,
                    split_k=info.split_k, ring=ring, arm=arm, us=round(t, 2), weight_bytes=wbytes,
                    weight_gbps=round(wbytes / t / 1e3, 1), frac=round(wbytes / (t * 1e-6) / READ_CEILING, 3),
                    copies=copies, reps=15, out_sha1=digest))
                print(line, flush=True)
                with open(out, "a") as f:
                    f.write(line + "\n")
            del arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_mxfp4_ring_ab.jsonl"))
    ap.add_argument("--rings", default="3,4,6,8,3")
    ap.add_argument("--limit", type=int, default=200, help="seconds per build (child process)")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        child(args.child, args.lib, args.out)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()
    for ring in (int(r) for r in args.rings.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(ring), "--out", args.out]
        if ring != 3:
            lib = os.path.join(ROOT, "tools", "probes", "tmp_libs", f"mxring{ring}.so")
            if not os.path.exists(lib):
                sys.exit(f"{lib} not found: tools/build_variant.sh mxring{ring} dense.hip -DSLM_LIN_MX_RING={ring}")
            cmd += ["--lib", lib]
        try:
            rc = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.DEVNULL).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"[ab_mxfp4_ring] ring {ring} ended with {rc}: nothing more is started", file=sys.stderr)
            sys.exit(rc if rc > 0 else 1)
    rows = {}
    for line in open(args.out):
        r = json.loads(line)
        rows.setdefault((r["shape"], r["M"]), []).append((r["ring"], r["us"], r["out_sha1"]))
    for key, v in rows.items():
        same = len({h for _, _, h in v}) == 1
        print(key, " ".join(f"r{ring}:{us}" for ring, us, _ in v), "same bits" if same else "BITS DIFFER")


if __name__ == "__main__":
    main()
