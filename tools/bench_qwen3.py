"""The QK-norm prologue (slm_qk_norm_rope_kv_append, include/slm_hip.h section 19) and the Qwen3 / Qwen3-MoE decode
steps, measured at Qwen3-8B attention shapes (32 query / 8 KV heads of 128), bf16.  Everything is captured once in a
hipGraph and replayed `--iters` times between device events, in one process; every figure is the median of
`--repeats` such windows, listed with their spread (max - min).

    python tools/bench_qwen3.py [--out profiles/r21_qwen3.jsonl] [--iters 200] [--repeats 5] [--parts prologue,step]

  prologue  kernels.qk_norm_rope_kv_append alone against the captured composition of the entry points that existed
            before it, T = 1 / 32 / 256, both forms.  Plain form: contiguous copies of the q and k column slices of
            the fused qkv row -> rms_norm on [T * 32, 128] and [T * 8, 128] rows -> slm_rope_kv_append with the
            append (q and k stay in the dense copies, where attention can read them).  Slab form (4 slabs): torch's sum
            over the slabs rounded to bf16 into the row first (the reduce the deferred GEMM skipped), then the same.
  step      Qwen3DecodeStep cut to 8 layers, kv 4096, batch 1 and 32, for the dense Qwen3-8B shape and the
            Qwen3-30B-A3B MoE shape; each also with every handler forced onto the composition
            (set_qk_norm_fused(False): the qkv GEMM then reduces its own slabs).
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalellm_amd import kernels  # noqa: E402
from scalellm_amd.decode import make_decode_inputs  # noqa: E402
from scalellm_amd.qwen3 import Qwen3DecodeStep, Qwen3Shape  # noqa: E402

BF16 = torch.bfloat16
TOKENS = (1, 32, 256)
H, KV, D, EPS = 32, 8, 128, 1e-6


def _window(fn, iters):
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


def _measure(fns, args):
    """alternating windows over the candidates (drift hits all alike) -> per candidate (median us, spread us)"""
    t = [[] for _ in fns]
    for _ in range(args.repeats):
        for i, fn in enumerate(fns):
            t[i].append(_window(fn, args.iters))
    return [(round(sorted(v)[len(v) // 2], 2), round(max(v) - min(v), 2)) for v in t]


def _graph(body):
    body()                                     # warm-up: workspaces, lazy repacks
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    return g


def composed_prologue(q, k, v, qw, kw, pos, table, slots, kc, vc, scratch):
    """what the prologue replaces, from the entry points that existed before it"""
    qn, kn = scratch
    qn.copy_(q)
    kn.copy_(k)
    kernels.rms_norm(qn.view(-1, D), qn.view(-1, D), qw, EPS)
    kernels.rms_norm(kn.view(-1, D), kn.view(-1, D), kw, EPS)
    kernels.apply_rotary_pos_emb(qn, kn, pos, table, D, False, value=v, slot_ids=slots, key_cache=kc, value_cache=vc)


# ---- (i) the prologue alone -----------------------------------------------------------------------------------------
def part_prologue(args, dev):
    lines = []
    gen = torch.Generator(device=dev).manual_seed(1)
    n_slots, N = 8192, (H + 2 * KV) * D
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float32, device=dev) / D))
    ang = torch.arange(4096, dtype=torch.float32, device=dev)[:, None] * inv[None, :]
    table = torch.cat([ang.cos(), ang.sin()], dim=-1).contiguous()
    qw, kw = ((1 + 0.1 * torch.randn(D, device=dev, generator=gen)).to(BF16) for _ in range(2))
    kc, vc = (torch.zeros(n_slots, KV, D, device=dev, dtype=BF16) for _ in range(2))
    for T in TOKENS:
        row = torch.randn(T, N, device=dev, dtype=BF16, generator=gen)
        q, k, v = row[:, :H * D].view(T, H, D), row[:, H * D:(H + KV) * D].view(T, KV, D), \
            row[:, (H + KV) * D:].view(T, KV, D)
        pos = torch.randint(0, 4096, (T,), device=dev, dtype=torch.int32, generator=gen)
        slots = torch.randperm(n_slots, device=dev, generator=gen)[:T].to(torch.int32)
        scratch = (torch.empty(T, H, D, device=dev, dtype=BF16), torch.empty(T, KV, D, device=dev, dtype=BF16))
        slabs = (torch.randn(4, T, N, device=dev, generator=gen) * 0.5).contiguous()
        part = kernels.DeferredPartials.from_slabs(slabs)

        def fused_plain():
            kernels.qk_norm_rope_kv_append(q, k, v, qw, kw, EPS, pos, table, False, slot_ids=slots, key_cache=kc,
                                           value_cache=vc)

        def fused_slabs():
            kernels.qk_norm_rope_kv_append(q, k, v, qw, kw, EPS, pos, table, False, slot_ids=slots, key_cache=kc,
                                           value_cache=vc, partials=part)

        def composed_plain():
            composed_prologue(q, k, v, qw, kw, pos, table, slots, kc, vc, scratch)

        def composed_slabs():
            row.copy_(slabs.sum(0))
            composed_prologue(q, k, v, qw, kw, pos, table, slots, kc, vc, scratch)
        for form, fused, comp in (("plain", fused_plain, composed_plain), ("slabs", fused_slabs, composed_slabs)):
            gf, gc = _graph(fused), _graph(comp)
            (f_us, f_sp), (c_us, c_sp) = _measure([lambda i: gf.replay(), lambda i: gc.replay()], args)
            line = dict(bench="qk_norm_rope_kv_append", form=form, T=T, n_heads=H, n_kv_heads=KV, head_dim=D,
                        n_splits=4 if form == "slabs" else 0, kernel_us=f_us, kernel_spread_us=f_sp,
                        composition_us=c_us, composition_spread_us=c_sp, kernel_over_composition=round(f_us / c_us, 3),
                        iters=args.iters, repeats=args.repeats)
            print(json.dumps(line), flush=True)
            lines.append(line)
    return lines


# ---- (ii) the step --------------------------------------------------------------------------------------------------
def part_step(args, dev):
    lines = []
    kv_len, block = 4096, 16
    for kind, preset in (("dense", Qwen3Shape.qwen3_8b), ("moe", Qwen3Shape.qwen3_30b_a3b)):
        shape = dataclasses.replace(preset(), n_layers=8, max_position=8192)
        nb = make_decode_inputs(32, kv_len, block, dev, vocab=shape.vocab)[3]
        step = Qwen3DecodeStep(shape, 32, nb, block, device=dev)
        for L in step.layers:
            for t in L["kv"].get_kv_cache():
                t.normal_()
        for bs in (1, 32):
            tokens, positions, params, _ = make_decode_inputs(bs, kv_len, block, dev, seed=bs, vocab=shape.vocab)
            step.reserve_workspaces(bs, kv_len)
            graphs, deferred = [], []
            for fused in (True, False):
                step.set_qk_norm_fused(fused)
                graphs.append(_graph(lambda: step.forward(tokens, positions, params)))
                deferred.append(bool(step.layers[0]["qkv"].deferred))   # did the qkv GEMM leave slabs
            step.set_qk_norm_fused(True)
            gf, gc = graphs
            (f_us, f_sp), (c_us, c_sp) = _measure([lambda i: gf.replay(), lambda i: gc.replay()], args)
            line = dict(bench=f"qwen3_{kind}_step_8_layers", preset=preset.__name__, quant_method="none", batch=bs,
                        kv_len=kv_len, step_us=f_us, step_spread_us=f_sp, composed_step_us=c_us,
                        composed_step_spread_us=c_sp, step_over_composed=round(f_us / c_us, 4),
                        per_layer_us=round(f_us / shape.n_layers, 1), qkv_deferred=deferred[0],
                        composed_qkv_deferred=deferred[1],
                        iters=args.iters, repeats=args.repeats)
            print(json.dumps(line), flush=True)
            lines.append(line)
        del step, graphs, gf, gc
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="prologue,step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qwen3 needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda")
    lines = []
    for part in args.parts.split(","):
        lines += {"prologue": part_prologue, "step": part_step}[part](args, dev)
        if args.out:                                   # after every part: a later part's failure loses nothing
            with open(args.out, "w") as f:
                for line in lines:
                    f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
