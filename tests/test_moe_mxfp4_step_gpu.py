"""MixtralDecodeStep and Qwen3DecodeStep with quant_method="mxfp4" (attention projections -- and Qwen3's dense MLP -- on
layers.{Column,Row}ParallelMxfp4Linear, experts on moe.MoEMxfp4Experts, router / embedding / head / norms in T) against
the SAME step with quant_method="none" loaded with the dequantised checkpoint.  e2m1 * 2^(e - 127) is exact in bf16,
the MXFP4 linear takes the dense plan of the same (M, N, K, dtype, flags, bias) and the grouped GEMMs share their launch
shapes, so every MFMA sees the same values in the same order: logits, recorded routing and the appended KV are
bit-equal, with no tolerance.  A short schedule: one prefill step (four prompts of 5 to 40 tokens), two decode steps;
then a captured decode step replayed over changed lengths."""
import numpy as np
import pytest
import torch

from tests.e2e_common import Sequences

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
BLOCK = 16
PROMPTS = [5, 40, 12, 23]
DT = torch.bfloat16


def _family(name):
    from scalellm_amd.mixtral import MixtralDecodeStep, MixtralShape
    from scalellm_amd.qwen3 import Qwen3DecodeStep, Qwen3Shape
    return {"mixtral-tiny": (MixtralDecodeStep, MixtralShape.tiny()),
            "qwen3-tiny_moe": (Qwen3DecodeStep, Qwen3Shape.tiny_moe()),
            "qwen3-tiny": (Qwen3DecodeStep, Qwen3Shape.tiny())}[name]


def _params(inp, **kw):
    from scalellm_amd.layers import InputParameters
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return (t(inp["tokens"]), t(inp["positions"]),
            InputParameters(q_cu_seq_lens=t(inp["q_cu"]), kv_cu_seq_lens=t(inp["kv_cu"]),
                            new_cache_slots=t(inp["slots"]), block_tables=t(inp["table"]),
                            cu_block_lens=t(inp["bcu"]), q_max_seq_len=inp["max_q"], kv_max_seq_len=inp["max_kv"], **kw))


def _pair(name, seqs, seed):
    """(the mxfp4 step, the unquantised step of the same seed carrying the mxfp4 step's weights dequantised)"""
    from scalellm_amd import kernels, layers, moe
    cls, shape = _family(name)
    moe_shape = bool(getattr(shape, "n_experts", 0))
    kw = dict(dtype=DT, device=DEV, seed=seed, keep_checkpoint=True, record_routing=moe_shape)
    T = sum(PROMPTS) + 8
    mx = cls(shape, T, seqs.n_blocks, BLOCK, quant_method="mxfp4", **kw)
    dense = cls(shape, T, seqs.n_blocks, BLOCK, quant_method="none", **kw)
    linears = [n for n in ("qkv", "o", "gate_up", "down") if n in mx.layers[0]]
    assert linears == (["qkv", "o"] if moe_shape else ["qkv", "o", "gate_up", "down"])
    for li, (Lm, Ld) in enumerate(zip(mx.layers, dense.layers)):
        for n in linears:
            col = n in ("qkv", "gate_up")
            assert type(Lm[n]) is (layers.ColumnParallelMxfp4Linear if col else layers.RowParallelMxfp4Linear)
            assert type(Ld[n]) is (layers.ColumnParallelLinear if col else layers.RowParallelLinear)
            # the mxfp4 checkpoint is the "none" checkpoint of the same seed quantised, under the Quark names
            ck = mx.ckpt[li][n]
            assert sorted(ck) == ["weight", "weight_scale"] and ck["weight"].dtype == torch.uint8
            w4, sc = kernels.quantize_mxfp4_weight(dense.ckpt[li][n]["weight"])
            assert torch.equal(w4, Lm[n].weight) and torch.equal(sc, Lm[n].weight_scale), (li, n)
            assert int(sc.min()) >= 2 and int(sc.max()) <= 252                         # bf16's exact range
            Ld[n].weight = kernels.dequantize_mxfp4_weight(w4, sc, DT).contiguous()
        if moe_shape:
            em, ed = Lm["moe"].experts, Ld["moe"].experts
            assert type(em) is moe.MoEMxfp4Experts and type(ed) is moe.MoEDenseExperts
            assert torch.equal(Lm["moe"].gate_weight, Ld["moe"].gate_weight) and Lm["moe"].gate_weight.dtype == DT
            sd = mx.ckpt[li]["moe"]
            assert sd["experts.0.w1.weight"].dtype == torch.uint8 and "experts.0.w2.weight_scale" in sd
            for which in ("gate_up", "down"):
                p, s = getattr(em, which), getattr(em, which + "_scale")
                assert int(s.min()) >= 2 and int(s.max()) <= 252
                E, N = p.shape[:2]
                deq = kernels.dequantize_mxfp4_weight(p.view(E * N, -1), s.view(E * N, -1), DT).view(E, N, -1)
                assert deq.shape == getattr(ed, which).shape
                setattr(ed, which, deq.contiguous())
        for n in ("in_norm", "post_norm") + (("q_norm", "k_norm") if "q_norm" in Lm else ()):
            assert torch.equal(Lm[n], Ld[n]) and Lm[n].dtype == DT
    assert torch.equal(mx.embed, dense.embed) and torch.equal(mx.lm_head, dense.lm_head) and mx.embed.dtype == DT
    return mx, dense


@pytest.fixture(scope="module", params=["mixtral-tiny", "qwen3-tiny_moe", "qwen3-tiny"])
def pair(request):
    """both steps after the schedule, run once per family: (name, mx, dense, seqs, records)"""
    name = request.param
    seqs = Sequences(PROMPTS, 8, BLOCK, 1024, seed=13)
    mx, dense = _pair(name, seqs, seed=4)
    records = []
    for new_lens in (list(PROMPTS), [1] * len(PROMPTS), [1] * len(PROMPTS)):
        inp = seqs.inputs(new_lens)
        T = sum(new_lens)
        rec = {}
        for what, model in (("mx", mx), ("dense", dense)):
            tokens, positions, params = _params(inp)
            rec[what] = model.forward(tokens, positions, params, return_logits=True).clone()
            torch.cuda.synchronize()
            if model.routing is not None:
                rec[what + "_routing"] = [{k: r[k][:T].clone() for k in ("logits", "indices", "weights")}
                                          for r in model.routing]
        records.append(rec)
        seqs.advance(new_lens)
        seqs.feed(inp, rec["mx"].float().cpu().numpy().argmax(-1))
    return name, mx, dense, seqs, records


def test_logits_routing_and_kv_equal_the_dense_step_on_the_dequantised_checkpoint(pair):
    name, mx, dense, seqs, records = pair
    assert len(records) == 3
    for si, rec in enumerate(records):
        got, want = rec["mx"], rec["dense"]
        assert got.shape == (len(PROMPTS), mx.shape.vocab) and bool(torch.isfinite(got.float()).all())
        assert float(got.float().abs().max()) > 0
        assert torch.equal(got, want), (name, si, float((got.float() - want.float()).abs().max()))
        if "mx_routing" in rec:
            assert len(rec["mx_routing"]) == mx.shape.n_layers
            for li, (rm, rd) in enumerate(zip(rec["mx_routing"], rec["dense_routing"])):
                for k in ("logits", "indices", "weights"):
                    assert torch.equal(rm[k], rd[k]), (name, si, li, k)
                assert int(rm["indices"].min()) >= 0 and int(rm["indices"].max()) < mx.shape.n_experts
    assert not torch.equal(records[1]["mx"], records[2]["mx"])
    # ... and the same KV was appended, at every slot the schedule wrote (the rest of a cache is uninitialised)
    slots = torch.tensor([int(seqs.blocks[s][i // BLOCK]) * BLOCK + i % BLOCK
                          for s in range(len(PROMPTS)) for i in range(PROMPTS[s] + 2)], device=DEV)
    assert slots.numel() == sum(PROMPTS) + 2 * len(PROMPTS) == slots.unique().numel()
    for Lm, Ld in zip(mx.layers, dense.layers):
        assert torch.equal(Lm["kv"].key_cache[slots], Ld["kv"].key_cache[slots])
        assert torch.equal(Lm["kv"].value_cache[slots], Ld["kv"].value_cache[slots])
        assert bool(torch.isfinite(Lm["kv"].key_cache[slots].float()).all())


def test_the_experts_holder_is_the_mxfp4_class(pair):
    from scalellm_amd import moe
    name, mx, _, _, _ = pair
    assert mx.quant_method == "mxfp4"
    if name == "qwen3-tiny":
        assert all("moe" not in L and L["gate_up"].paired for L in mx.layers)     # dense MLP, SiLU * mul in the epilogue
        return
    s = mx.shape
    inter = getattr(s, "moe_intermediate", 0) or s.intermediate
    for L in mx.layers:
        ex = L["moe"].experts
        assert isinstance(ex, moe.MoEMxfp4Experts)
        assert tuple(ex.gate_up.shape) == (s.n_experts, 2 * inter, s.hidden // 2)
        assert tuple(ex.down_scale.shape) == (s.n_experts, s.hidden, inter // 32)
        assert ex.nbytes() == 3 * s.n_experts * s.hidden * inter * 17 // 32      # 4.25 bits a weight


def test_captured_decode_step_replays_over_changed_lengths(pair):
    from scalellm_amd.layers import InputParameters
    _, model, _, seqs, _ = pair
    n = len(PROMPTS)
    ones = [1] * n
    inp = seqs.inputs(ones)
    # static inputs, the block table at its full length (every sequence's blocks for the steps to come)
    full_table = np.concatenate([seqs.blocks[s] * BLOCK for s in range(n)]).astype(np.int32)
    bcu = np.concatenate([[0], np.cumsum([len(seqs.blocks[s]) for s in range(n)])]).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    st = dict(tokens=t(inp["tokens"]), positions=t(inp["positions"]), q_cu=t(inp["q_cu"]), kv_cu=t(inp["kv_cu"]),
              slots=t(inp["slots"]))
    params = InputParameters(q_cu_seq_lens=st["q_cu"], kv_cu_seq_lens=st["kv_cu"], new_cache_slots=st["slots"],
                             block_tables=t(full_table), cu_block_lens=t(bcu), q_max_seq_len=1,
                             kv_max_seq_len=max(len(b) for b in seqs.blocks) * BLOCK, kv_total_len=-1)
    model.reserve_workspaces(n, params.kv_max_seq_len)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm-up (writes this step's KV: harmless, the
        model.forward(st["tokens"], st["positions"], params, return_logits=True)   # replay writes the same rows)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        logits = model.forward(st["tokens"], st["positions"], params, return_logits=True)
    seen = []
    for rep in range(2):                                           # two steps: the lengths change under the graph
        inp = seqs.inputs(ones)
        for k in ("tokens", "positions", "q_cu", "kv_cu", "slots"):
            st[k].copy_(t(inp[k]))
        graph.replay()
        torch.cuda.synchronize()
        got = logits.float().cpu().numpy()
        eager = model.forward(st["tokens"], st["positions"], params, return_logits=True).float().cpu().numpy()
        assert np.isfinite(got).all()
        assert np.array_equal(got, eager), "the replay differs from the eager step on the same inputs"
        seen.append(got)
        seqs.advance(ones)
        seqs.feed(inp, got.argmax(-1))
    assert not np.array_equal(seen[0], seen[1])


def test_methods_accepted_before_are_what_they_were():
    """"none" still builds the unquantised classes; an unknown method is still a ValueError naming the accepted ones"""
    from scalellm_amd import layers, moe
    for name in ("mixtral-tiny", "qwen3-tiny_moe"):
        cls, shape = _family(name)
        m = cls(shape, 8, 4, BLOCK, quant_method="none", dtype=DT, device=DEV)
        assert type(m.layers[0]["qkv"]) is layers.ColumnParallelLinear
        assert type(m.layers[0]["moe"].experts) is moe.MoEDenseExperts
        with pytest.raises(ValueError, match="'none', 'fp8', 'awq' or 'mxfp4'"):
            cls(shape, 8, 4, BLOCK, quant_method="int3", dtype=DT, device=DEV)
