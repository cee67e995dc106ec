"""Qwen3DecodeStep (scalellm_amd/qwen3.py) end to end against tests/qwen3_model_ref.py (the torch-fp32 restatement of
the Qwen3 / Qwen3-MoE forwards, pinned on HuggingFace by tests/test_qwen3_ref_cpu.py) on the step's own checkpoint,
dequantised where it is quantised: a prefill step of three prompts, then decode steps along the reference's greedy
path.  bf16, Qwen3Shape.tiny() (hidden 256, 8 heads x 64, 2 KV heads, intermediate 512, 2 layers, vocab 1024) and
tiny_moe() (8 experts, top 2, expert intermediate 128); block 16.

The method and the bound are tests/test_mixtral_step_gpu.py's: check_logits at 3e-2 for every quant_method, and for
the MoE shape the GPU's recorded expert ids forced into the reference (which computes its own weights at them).

Beside that: a captured decode step replays bit for bit as the eager one; the step with the fused QK-norm prologue is
bit-equal to the same step with every handler forced onto the composition of the older entry points; the step with
deferred split-K slabs (SLM_DEFER_SPLITK) agrees with the one without within the bound; a tied head.  At these sizes
the dense GEMMs do not split K on their own, so the tests of the slab form force two K slices (SLM_LINEAR_SPLITK=2)
and check that the qkv slabs were deferred."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import qwen3_model_ref as R
from tests.e2e_common import Sequences, check_logits, rel_l2
from tests.test_mixtral_step_gpu import _Routing, _dense_nk, _params

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
TOL = 3e-2
BLOCK, GROUP = 16, 128
PROMPTS = [5, 17, 12]
N_DECODE = 3


def _shape(kind, tied=False):
    from scalellm_amd.qwen3 import Qwen3Shape
    s = Qwen3Shape.tiny_moe() if kind == "moe" else Qwen3Shape.tiny()
    return dataclasses.replace(s, tie_word_embeddings=tied)


def _model(kind, quant_method="none", tied=False, seed=3):
    from scalellm_amd.qwen3 import Qwen3DecodeStep
    shape = _shape(kind, tied)
    seqs = Sequences(PROMPTS, N_DECODE + 4, BLOCK, shape.vocab, seed=13)
    model = Qwen3DecodeStep(shape, sum(PROMPTS) + 8, seqs.n_blocks, BLOCK, quant_method=quant_method,
                            group_size=GROUP, dtype=torch.bfloat16, device=DEV, seed=seed, keep_checkpoint=True,
                            record_routing=kind == "moe")
    return model, seqs


def _reference(model):
    """the restatement over the step's own checkpoint, its norm weights, embedding and lm_head"""
    f = lambda t: t.float().cpu()  # noqa: E731
    s = model.shape
    layers = []
    for li, ck in enumerate(model.ckpt):
        L = model.layers[li]
        W = {"qkv": _dense_nk(ck["qkv"], model.dtype).t().contiguous(),
             "o": _dense_nk(ck["o"], model.dtype).t().contiguous(), "q_norm": f(L["q_norm"]),
             "k_norm": f(L["k_norm"]), "in_norm": f(L["in_norm"]), "post_norm": f(L["post_norm"])}
        if s.n_experts:
            sd = ck["moe"]
            expert = lambda e, w: _dense_nk({k[len(f"experts.{e}.{w}."):]: v for k, v in sd.items()  # noqa: E731
                                             if k.startswith(f"experts.{e}.{w}.")}, model.dtype)
            W["gate"] = f(sd["gate.weight"])
            for w in ("w1", "w3", "w2"):
                W[w] = torch.stack([expert(e, w) for e in range(s.n_experts)]).contiguous()
        else:
            gu = _dense_nk(ck["gate_up"], model.dtype)             # [2 I, H]: gate rows, then up rows
            W["w1"], W["w3"] = gu[:s.intermediate].contiguous(), gu[s.intermediate:].contiguous()
            W["w2"] = _dense_nk(ck["down"], model.dtype).contiguous()
        layers.append(W)
    return R.Qwen3Ref(layers, f(model.final_norm), f(model.embed), f(model.lm_head), R.Qwen3RefConfig(
        n_heads=s.n_heads, n_kv_heads=s.n_kv_heads, head_dim=s.head_dim, topk=s.topk, rms_eps=s.rms_eps,
        rope_theta=s.rope_theta, renormalize=s.norm_topk_prob, n_experts=s.n_experts))


def _steps():
    return [list(PROMPTS)] + [[1] * len(PROMPTS)] * N_DECODE


def _ref_rows(ref, seqs, new_lens, routing):
    rows = []
    for s, n in enumerate(new_lens):
        c = seqs.cached[s]
        forced = routing.forced(s) if routing is not None else None
        rows.append(ref.logits(seqs.tokens[s][:c + n], forced=forced)[-1].numpy())
    return np.stack(rows)


def _run_against_reference(model, seqs, what):
    ref = _reference(model)
    routing = _Routing(len(PROMPTS), model.shape.n_layers) if model.shape.n_experts else None
    for si, new_lens in enumerate(_steps()):
        inp = seqs.inputs(new_lens)
        tokens, positions, params = _params(inp)
        got = model.forward(tokens, positions, params, return_logits=True).float().cpu().numpy()
        if routing is not None:
            routing.record(model, new_lens)
        want = _ref_rows(ref, seqs, new_lens, routing)
        a, n, rel = check_logits(got, want, TOL, f"{what} step {si}")
        print(f"\n[qwen3-step] {what} step {si} q_lens {new_lens}: rel L2 {rel:.4f}, greedy {a}/{n}")
        seqs.advance(new_lens)
        seqs.feed(inp, want.argmax(-1))                            # the REFERENCE's greedy path
    return ref


@pytest.mark.parametrize("quant_method", ["none", "fp8", "awq"])
@pytest.mark.parametrize("kind", ["dense", "moe"])
def test_steps_match_the_reference(kind, quant_method):
    model, seqs = _model(kind, quant_method)
    if kind == "moe":
        from scalellm_amd import moe
        want = {"none": moe.FusedMoE, "fp8": moe.MoEFp8Experts, "awq": moe.MoEQuantExperts}[quant_method]
        assert quant_method == "none" or isinstance(model.layers[0]["moe"].experts, want)
    assert model.layers[0]["attn"].handler.q_norm is model.layers[0]["q_norm"]
    ref = _run_against_reference(model, seqs, f"{kind} {quant_method}")
    if kind == "dense" and quant_method == "none":
        # the comparison sees the QK norm: the restatement without it misses the same GPU logits by more than the bound
        inp = seqs.inputs([1] * len(PROMPTS))
        tokens, positions, params = _params(inp)
        got = model.forward(tokens, positions, params, return_logits=True).float().cpu().numpy()
        want = _ref_rows(ref, seqs, [1] * len(PROMPTS), None)
        off = _ref_rows(ref.variant(qk_norm=False), seqs, [1] * len(PROMPTS), None)
        print(f"\n[qwen3-step] control without the QK norm: rel L2 {rel_l2(got, off):.4f} (bound {TOL})")
        assert rel_l2(got, want) <= TOL < rel_l2(got, off)


def test_tied_head_matches_the_reference():
    model, seqs = _model("dense", "none", tied=True)
    assert model.lm_head.data_ptr() == model.embed.data_ptr()
    _run_against_reference(model, seqs, "dense tied")


def _forward_steps(model, seqs, steps):
    out = []
    for new_lens in steps:
        inp = seqs.inputs(new_lens)
        tokens, positions, params = _params(inp)
        out.append(model.forward(tokens, positions, params, return_logits=True).float().cpu().numpy())
        seqs.advance(new_lens)
        seqs.feed(inp, out[-1].argmax(-1))
    return out


@pytest.mark.parametrize("kind", ["dense", "moe"])
def test_fused_prologue_is_bit_equal_to_the_composition(kind):
    """every step twice on the same inputs: fused (over the deferred qkv slabs), then every handler on copies + two
    rms_norm + apply_rotary_pos_emb after the qkv GEMM's own reduce.  The KV rows the second run writes are the rows
    the first wrote (when the bits agree, which is what is asserted)."""
    from scalellm_amd import kernels
    model, seqs = _model(kind)
    assert model.defer_splitk
    with kernels.tuning(SLM_LINEAR_SPLITK=2):
        for new_lens in _steps():
            inp = seqs.inputs(new_lens)
            tokens, positions, params = _params(inp)
            got = []
            for fused in (True, False):
                model.set_qk_norm_fused(fused)
                got.append(model.forward(tokens, positions, params, return_logits=True).float().cpu().numpy())
                assert bool(model.layers[0]["qkv"].deferred) == fused   # the slab form ran, or no slabs were left
            model.set_qk_norm_fused(True)
            assert np.isfinite(got[0]).all() and np.array_equal(got[0], got[1]), new_lens
            seqs.advance(new_lens)
            seqs.feed(inp, got[0].argmax(-1))


@pytest.mark.parametrize("kind", ["dense", "moe"])
def test_deferred_slabs_on_and_off_agree(kind, monkeypatch):
    from scalellm_amd import kernels
    runs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("SLM_DEFER_SPLITK", flag)
        model, seqs = _model(kind)
        assert model.defer_splitk == (flag == "1")
        with kernels.tuning(SLM_LINEAR_SPLITK=2):
            runs.append(_forward_steps(model, seqs, _steps()))
            assert bool(model.layers[0]["qkv"].deferred) == (flag == "1")
    for si, (a, b) in enumerate(zip(*runs)):
        rel = rel_l2(a, b)
        print(f"\n[qwen3-step] {kind} step {si}: deferred vs reduced rel L2 {rel:.2e}")
        assert rel <= TOL


@pytest.mark.parametrize("kind", ["dense", "moe"])
def test_captured_decode_step_replays_bit_equal_to_eager(kind):
    from scalellm_amd.layers import InputParameters
    model, seqs = _model(kind)
    _forward_steps(model, seqs, [list(PROMPTS)])
    n = len(PROMPTS)
    ones = [1] * n
    inp = seqs.inputs(ones)
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
    for _ in range(2):                                             # two steps: the lengths change under the graph
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
