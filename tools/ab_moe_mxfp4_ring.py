#!/usr/bin/env python3
"""A/B of the ring depth of moe_gemm.hip's mxfp4 weight side (SLM_MG_MX_RING), the grouped twin of
tools/ab_mxfp4_ring.py.

    for r in 4 6; do tools/build_variant.sh mgring$r moe_gemm.hip -DSLM_MG_MX_RING=$r; done
    python tools/ab_moe_mxfp4_ring.py [--out profiles/r23_moe_mxfp4_ring_ab.jsonl] [--rings 3,4,6,3]

One child process per library build -- ring 3 is the tree's libslm_hip.so, ring R tools/probes/tmp_libs/mgring<R>.so --
one after the other on one machine; the default order ends with the tree's build again, so the two ring-3 runs show
the drift between processes.  Per build: the MXFP4 layer of tools/bench_moe.py --mxfp4 (Mixtral-8x7B FusedMoE, graph
replay over a pool of inputs, the routing changing per replay) at T = 1 / 32 / 256, three windows of `--iters` replays.
One JSON line per T: kind "moe_ring_ab", `ring`, the windows, their median, and `out_sha1`, the digest of one output --
equal across the builds of a row, since no result bit depends on the depth.  A child that fails or overruns ends the
run."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def child(ring, lib, out, iters):
    import torch
    from scalellm_amd import _lib
    if lib:
        _lib.LIB_PATH = lib                                  # before the first call loads the library
    import bench_moe as B
    if not torch.cuda.is_available():
        sys.exit("ab_moe_mxfp4_ring needs a GPU: there is no CPU fallback")
    dev = torch.device("cuda")
    tokens = (1, 32, 256)
    (layer,) = B._mxfp4_fp8_and_dense_layers(max(tokens), dev, sides=("mxfp4",))
    for T in tokens:
        g = torch.Generator(device=dev).manual_seed(T)
        pool = [torch.randn(T, B.HID, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(16)]
        run, y = B._captured(layer, pool, T, dev)
        windows = [round(B._time(run, iters), 2) for _ in range(3)]
        digest = hashlib.sha1(y.view(torch.int16).cpu().numpy().tobytes()).hexdigest()[:12]
        line = json.dumps(dict(kind="moe_ring_ab", bench="moe_mixtral_8x7b_mxfp4_bf16", T=T, ring=ring,
                               us=sorted(windows)[1], us_windows=windows, iters=iters, pool=16, out_sha1=digest))
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_moe_mxfp4_ring_ab.jsonl"))
    ap.add_argument("--rings", default="3,4,6,3")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--limit", type=int, default=200, help="seconds per build (child process)")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        child(args.child, args.lib, args.out, args.iters)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()
    for ring in (int(r) for r in args.rings.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(ring), "--out", args.out, "--iters",
               str(args.iters)]
        if ring != 3:
            lib = os.path.join(ROOT, "tools", "probes", "tmp_libs", f"mgring{ring}.so")
            if not os.path.exists(lib):
                sys.exit(f"{lib} not found: tools/build_variant.sh mgring{ring} moe_gemm.hip -DSLM_MG_MX_RING={ring}")
            cmd += ["--lib", lib]
        try:
            rc = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.DEVNULL).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"[ab_moe_mxfp4_ring] ring {ring} ended with {rc}: nothing more is started", file=sys.stderr)
            sys.exit(rc if rc > 0 else 1)
    rows = {}
    for line in open(args.out):
        r = json.loads(line)
        rows.setdefault(r["T"], []).append((r["ring"], r["us"], r["out_sha1"]))
    for key, v in rows.items():
        same = len({h for _, _, h in v}) == 1
        print("T", key, " ".join(f"r{ring}:{us}" for ring, us, _ in v), "same bits" if same else "BITS DIFFER")


if __name__ == "__main__":
    main()
