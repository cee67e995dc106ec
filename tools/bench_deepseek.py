"""The MLA prologue (slm_mla_rope_append, include/slm_hip.h section 18), the shared-expert sum (slm_moe_sum_add) and the
DeepSeek-V2 decode step, measured at DeepSeek-V2-Lite shapes (16 heads, 128 + 64, v 128, latent 512, hidden 2048,
64 routed + 2 shared experts of 1408, top 6), bf16.  Everything is captured once in a hipGraph and replayed `--iters`
times between device events, in one process; every figure is the median of `--repeats` such windows, listed with
their spread (max - min).

    python tools/bench_deepseek.py [--out profiles/r20_deepseek.jsonl] [--iters 200] [--repeats 5] [--parts append,attn,moe,step]

  append  kernels.mla_rope_append alone against the captured composition of the entry points that existed before it,
          T = 1 / 32 / 256, both forms.  Plain form: a contiguous copy of the latent columns -> rms_norm; a copy of the
          query tails and the key into 64-wide heads -> slm_rope_kv_append -> a copy of the tails back; then
          mla_set_kv_cache.  Slab form (4 slabs): torch's sum over the slabs rounded to bf16 first, then the same.
  attn    layers.MLAAttention.forward (projection, prologue, q absorb, paged attention, v up, o) on decode rows,
          kv 4096, batch 1 / 32.
  moe     the sparse layer with its shared experts: FusedMoE(shared_out=) against FusedMoE() + a torch add,
          T = 1 / 32 / 256.
  step    DeepseekV2DecodeStep at the V2-Lite shape cut to 8 of its 27 layers, kv 4096, batch 1 and 32.
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalellm_amd import kernels, moe  # noqa: E402
from scalellm_amd.decode import make_decode_inputs  # noqa: E402
from scalellm_amd.deepseek import DeepseekV2DecodeStep, DeepseekV2Shape  # noqa: E402

BF16 = torch.bfloat16
TOKENS = (1, 32, 256)
H, NOPE, ROPE, LATENT, EPS = 16, 128, 64, 512, 1e-6
QK = NOPE + ROPE


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
    body()                                     # warm-up: workspaces, lazy repacks, index lists
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    return g


def composed_append(q, kv_a, w, pos, table, slots, kvc, krc, scratch):
    """what the prologue replaces, from the entry points that existed before it"""
    c, n, heads, dummy = scratch
    T = q.size(0)
    c.copy_(kv_a[:, :LATENT])
    kernels.rms_norm(n, c, w, EPS)
    heads[:, :H].copy_(q[:, :, NOPE:])
    heads[:, H].copy_(kv_a[:, LATENT:])
    kernels.apply_rotary_pos_emb(heads, dummy, pos, table, ROPE, True)
    q[:, :, NOPE:].copy_(heads[:, :H])
    kernels.mla_set_kv_cache(slots, n, heads[:, H], kvc, krc)
    return T


# ---- (i) the prologue alone -----------------------------------------------------------------------------------------
def part_append(args, dev):
    lines = []
    gen = torch.Generator(device=dev).manual_seed(1)
    n_slots, N = 8192, H * QK + LATENT + ROPE
    inv = 1.0 / (10000.0 ** (torch.arange(0, ROPE, 2, dtype=torch.float32, device=dev) / ROPE))
    ang = torch.arange(4096, dtype=torch.float32, device=dev)[:, None] * inv[None, :]
    table = torch.cat([ang.cos(), ang.sin()], dim=-1).contiguous()
    w = (1 + 0.1 * torch.randn(LATENT, device=dev, generator=gen)).to(BF16)
    kvc, krc = torch.zeros(n_slots, LATENT, device=dev, dtype=BF16), torch.zeros(n_slots, ROPE, device=dev, dtype=BF16)
    for T in TOKENS:
        row = torch.randn(T, N, device=dev, dtype=BF16, generator=gen)
        q, kv_a = row[:, :H * QK].view(T, H, QK), row[:, H * QK:]
        q_dense = torch.empty(T, H, QK, device=dev, dtype=BF16)
        pos = torch.randint(0, 4096, (T,), device=dev, dtype=torch.int32, generator=gen)
        slots = torch.randperm(n_slots, device=dev, generator=gen)[:T].to(torch.int32)
        scratch = (torch.empty(T, LATENT, device=dev, dtype=BF16), torch.empty(T, LATENT, device=dev, dtype=BF16),
                   torch.empty(T, H + 1, ROPE, device=dev, dtype=BF16), torch.zeros(T, 1, ROPE, device=dev, dtype=BF16))
        slabs = (torch.randn(4, T, N, device=dev, generator=gen) * 0.5).contiguous()
        part = kernels.DeferredPartials.from_slabs(slabs)

        def composed_slabs():
            row.copy_(slabs.sum(0))
            composed_append(q, kv_a, w, pos, table, slots, kvc, krc, scratch)
        for form, fused, comp in (
                ("plain", lambda: kernels.mla_rope_append(q, kv_a, w, EPS, pos, table, True, slots, kvc, krc, NOPE),
                 lambda: composed_append(q, kv_a, w, pos, table, slots, kvc, krc, scratch)),
                ("slabs", lambda: kernels.mla_rope_append(q_dense, None, w, EPS, pos, table, True, slots, kvc, krc, NOPE,
                                                          partials=part), composed_slabs)):
            gf, gc = _graph(fused), _graph(comp)
            (f_us, f_sp), (c_us, c_sp) = _measure([lambda i: gf.replay(), lambda i: gc.replay()], args)
            line = dict(bench="mla_rope_append", form=form, T=T, n_heads=H, nope=NOPE, latent=LATENT,
                        n_splits=4 if form == "slabs" else 0, kernel_us=f_us, kernel_spread_us=f_sp,
                        composition_us=c_us, composition_spread_us=c_sp, kernel_over_composition=round(f_us / c_us, 3),
                        iters=args.iters, repeats=args.repeats)
            print(json.dumps(line), flush=True)
            lines.append(line)
    return lines


# ---- (ii) the attention block ---------------------------------------------------------------------------------------
def part_attn(args, dev):
    lines = []
    shape = dataclasses.replace(DeepseekV2Shape.v2_lite(), n_layers=1, vocab=256, max_position=8192)
    kv_len, block = 4096, 16
    nb = make_decode_inputs(32, kv_len, block, dev, vocab=shape.vocab)[3]
    step = DeepseekV2DecodeStep(shape, 32, nb, block, device=dev)
    attn, cache = step.layers[0]["attn"], step.layers[0]["kv"]
    for t in cache.get_kv_cache():
        t.normal_()
    step.reserve_workspaces(32, kv_len)
    for bs in (1, 32):
        _, positions, params, _ = make_decode_inputs(bs, kv_len, block, dev, seed=bs, vocab=shape.vocab)
        x = torch.randn(bs, shape.hidden, device=dev, dtype=BF16)
        out = torch.empty(bs, shape.hidden, device=dev, dtype=BF16)
        g = _graph(lambda: attn.forward(x, positions, cache, params, out=out, defer_splitk=True))
        (us, sp), = _measure([lambda i: g.replay()], args)
        line = dict(bench="mla_attention_v2_lite", batch=bs, kv_len=kv_len, attention_us=us, attention_spread_us=sp,
                    qkv_a_deferred=bool(attn.qkv_a.deferred), o_deferred=bool(attn.o.deferred), iters=args.iters,
                    repeats=args.repeats)
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


# ---- (iii) the sparse layer with its shared experts -----------------------------------------------------------------
def part_moe(args, dev):
    lines = []
    s = DeepseekV2Shape.v2_lite()
    step = DeepseekV2DecodeStep(dataclasses.replace(s, n_layers=2, vocab=256, max_position=64), max(TOKENS), 4, 16,
                                device=dev)
    layer = step.layers[1]["moe"]
    assert isinstance(layer, moe.FusedMoE)
    for T in TOKENS:
        gen = torch.Generator(device=dev).manual_seed(T)
        pool = [torch.randn(T, s.hidden, device=dev, dtype=BF16, generator=gen) for _ in range(args.pool)]
        x = pool[0].clone()
        shared = torch.randn(T, s.hidden, device=dev, dtype=BF16, generator=gen)
        o_f, o_c = torch.empty_like(shared), torch.empty_like(shared)
        gf = _graph(lambda: layer.forward(x, out=o_f, shared_out=shared))

        def composed():
            layer.forward(x, out=o_c)
            o_c.add_(shared)
        gc = _graph(composed)

        def replay(g):
            def fn(i):
                x.copy_(pool[i % len(pool)])
                g.replay()
            return fn
        (f_us, f_sp), (c_us, c_sp) = _measure([replay(gf), replay(gc)], args)
        rel = float((o_f.float() - o_c.float()).abs().mean() / o_c.float().abs().mean())
        line = dict(bench="fused_moe_shared_out", T=T, n_experts=s.n_routed_experts, topk=s.topk, hidden=s.hidden,
                    moe_intermediate=s.moe_intermediate, shared_out_us=f_us, shared_out_spread_us=f_sp,
                    sum_then_add_us=c_us, sum_then_add_spread_us=c_sp, fused_over_composed=round(f_us / c_us, 4),
                    out_rel_diff=round(rel, 5), iters=args.iters, repeats=args.repeats, pool=args.pool)
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


# ---- (iv) the step --------------------------------------------------------------------------------------------------
def part_step(args, dev):
    lines = []
    shape = dataclasses.replace(DeepseekV2Shape.v2_lite(), n_layers=8, max_position=8192)
    kv_len, block = 4096, 16
    nb = make_decode_inputs(32, kv_len, block, dev, vocab=shape.vocab)[3]
    step = DeepseekV2DecodeStep(shape, 32, nb, block, device=dev)
    for L in step.layers:
        for t in L["kv"].get_kv_cache():
            t.normal_()
    for bs in (1, 32):
        tokens, positions, params, _ = make_decode_inputs(bs, kv_len, block, dev, seed=bs, vocab=shape.vocab)
        step.reserve_workspaces(bs, kv_len)
        g = _graph(lambda: step.forward(tokens, positions, params))
        (us, sp), = _measure([lambda i: g.replay()], args)
        line = dict(bench="deepseek_v2_lite_step_8_of_27_layers", quant_method="none", batch=bs, kv_len=kv_len,
                    step_us=us, step_spread_us=sp, per_layer_us=round(us / shape.n_layers, 1), iters=args.iters,
                    repeats=args.repeats)
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--parts", default="append,attn,moe,step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deepseek needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda")
    lines = []
    for part in args.parts.split(","):
        lines += {"append": part_append, "attn": part_attn, "moe": part_moe, "step": part_step}[part](args, dev)
        if args.out:                                   # after every part: a later part's failure loses nothing
            with open(args.out, "w") as f:
                for line in lines:
                    f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
