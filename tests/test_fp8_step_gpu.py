"""A Llama decode step over fp8 (e4m3) weights (LlamaDecodeStep(quant_method="fp8"): the four linears are
layers.{Column,Row}ParallelFp8Linear over slm_fp8_linear) against the oracle-composed fp32 forward and its
bf16-storage twin built from the DEQUANTISED weights (w8.float() * scale: quantisation is no error source), with the
bounds tests/test_dense_step_gpu.py uses; graph replay and repeatability, and a guard that the "none" and "awq"
steps did not move."""
import dataclasses

import numpy as np
import pytest
import torch

from tests.e2e_common import OracleLlama, Sequences, check_logits
from tests.test_dense_step_gpu import _filled, _params
from tests.test_model_runner_gpu import _batch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None


def _oracle_twin(model, storage=None):
    """The same model rebuilt on the CPU from the kept checkpoint: w8.float() * scale [N, K] -> the oracle's [K, N]"""
    s = model.shape
    f = lambda t: t.float().cpu().numpy()  # noqa: E731
    layers = []
    for li, ck in enumerate(model.ckpt):
        W = {}
        for n in ("qkv", "o", "gate_up", "down"):
            assert ck[n]["weight"].dtype == torch.float8_e4m3fn and ck[n]["weight_scale"].dtype == torch.float32
            W[n] = np.ascontiguousarray((f(ck[n]["weight"]) * f(ck[n]["weight_scale"])[:, None]).T)
        W["in_norm"], W["post_norm"] = f(model.layers[li]["in_norm"]), f(model.layers[li]["post_norm"])
        layers.append(W)
    D = s.head_dim
    inv_freq = (1.0 / (s.rope_theta ** (np.arange(0, D, 2, dtype=np.float32) / D))).astype(np.float32)
    return OracleLlama(layers, f(model.final_norm), f(model.embed), f(model.lm_head), s.n_heads, s.n_kv_heads, D,
                       s.rms_eps, inv_freq, model.block_size, model.layers[0]["kv"].key_cache.size(0), storage=storage)


def _step(quant_method, max_tokens, n_blocks, B, seed=3, **kw):
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape
    return LlamaDecodeStep(LlamaShape.tiny(), max_tokens, n_blocks, B, quant_method=quant_method, dtype=torch.bfloat16,
                           device=DEV, seed=seed, **kw)


@pytest.mark.parametrize("split", [None, 2], ids=["plan", "splitk2"])
def test_fp8_step_prefill_chunk_and_decode_match_the_oracle(split, tune):
    """split = 2: the tiny shape's K is too shallow for the plan to split, so the knob forces two slices: o / down /
    qkv then leave deferred (scaled) slabs for the RMSNorm and the RoPE + append kernel in every step"""
    from scalellm_amd.decode import hf_state_dict
    from scalellm_amd.layers import ColumnParallelFp8Linear, RowParallelFp8Linear
    B, n_seq = 16, 40
    prompt_lens = [30, 45, 20] + [3 + (7 * i) % 11 for i in range(n_seq - 3)]
    seqs = Sequences(prompt_lens, 4, B, 1024, seed=7)
    rest = [0] * (n_seq - 3)
    steps = [("prefill of 70 tokens over 3 sequences", [30, 20, 20] + rest),
             ("chunked continuation beside two decode rows", [1, 25, 1] + rest),
             ("decode at T = 3", [1, 1, 1] + rest),
             ("prefill of the other 37 sequences", [0, 0, 0] + prompt_lens[3:]),
             ("decode at T = 40", [1] * n_seq)]
    model = _step("fp8", sum(prompt_lens) + 8, seqs.n_blocks, B, keep_checkpoint=True)
    s = model.shape
    assert model.fp8 and model.weight_bits == 8 and not model.fold_norm and model.lanes_min == 0
    L0 = model.layers[0]
    assert isinstance(L0["qkv"], ColumnParallelFp8Linear) and isinstance(L0["down"], RowParallelFp8Linear)
    assert L0["gate_up"].paired and model.buf["gate_up"] is None            # the SiLU epilogue
    assert tuple(model.ckpt[0]["qkv"]["weight"].shape) == ((s.n_heads + 2 * s.n_kv_heads) * s.head_dim, s.hidden)
    assert tuple(model.ckpt[1]["down"]["weight_scale"].shape) == (s.hidden,)
    sd = hf_state_dict(model)                                               # *.weight (fp8) and *.weight_scale
    assert sd["model.layers.1.self_attn.k_proj.weight"].dtype == torch.float8_e4m3fn
    assert tuple(sd["model.layers.1.self_attn.k_proj.weight"].shape) == (s.n_kv_heads * s.head_dim, s.hidden)
    assert tuple(sd["model.layers.1.self_attn.k_proj.weight_scale"].shape) == (s.n_kv_heads * s.head_dim,)
    assert tuple(sd["model.layers.0.mlp.up_proj.weight_scale"].shape) == (s.intermediate,)
    assert not any(k.endswith(("qweight", "qzeros", "scales")) for k in sd)
    ref_model, twin_model = _oracle_twin(model), _oracle_twin(model, storage="bf16")
    rels, agree, total = [], 0, 0
    if split:
        tune(SLM_LINEAR_SPLITK=split)
    for what, new_lens in steps:
        inp = seqs.inputs(new_lens)
        tokens, positions, params = _params(inp)
        logits = model.forward(tokens, positions, params, return_logits=True)
        torch.cuda.synchronize()
        assert model.last_lanes == 1
        assert all(L0[n].deferred_splits == (split or 0) for n in ("qkv", "o", "down")) and not L0["gate_up"].deferred
        got = logits.float().cpu().numpy()
        a, n, rel = check_logits(got, ref_model.forward(inp), 3e-2, f"fp8, {what}: vs fp32 oracle")
        _, _, rel_t = check_logits(got, twin_model.forward(inp), 1.5e-2, f"fp8, {what}: vs bf16-storage twin")
        agree, total = agree + a, total + n
        rels.append((round(rel, 5), round(rel_t, 5)))
        seqs.advance(new_lens)
        seqs.feed(inp, got.argmax(-1))
    print(f"[fp8 e2e] per-step relative L2 error (vs fp32 oracle, vs bf16-storage twin): {rels}; "
          f"greedy ids equal on {agree}/{total} rows")
    assert model.defer_splitk


def test_fp8_decode_graph_replay_and_repeat_are_bit_identical():
    from scalellm_amd.model_runner import ModelRunner, ModelRunnerOptions
    B, max_len, n_blocks, bs = 16, 496, 400, 8
    model = _step("fp8", bs, n_blocks, B, seed=1)
    restore = _filled(model, 11)
    rng = np.random.default_rng(5)
    opts = ModelRunnerOptions(block_size=B, cuda_graph_max_seq_len=max_len, cuda_graph_batch_sizes=[bs],
                              num_decoding_tokens=1)
    runner = ModelRunner(model, DEV, opts, return_logits=True)
    runner.capture_cuda_graphs(bs)
    restore()
    for trial in range(2):                                   # the same graph over other (advanced) lengths
        kv = [int(x) for x in rng.integers(1 + 100 * trial, 150 + 100 * trial, size=bs)]
        t2, p2, prm2 = _batch(rng, bs, 1, kv, B, n_blocks, model.shape.vocab)
        hinted = dataclasses.replace(prm2, kv_max_seq_len=max_len)
        want = model.forward(t2, p2, hinted, return_logits=True).clone()
        restore()
        again = model.forward(t2, p2, hinted, return_logits=True).clone()   # a second identical step, same state
        restore()
        assert torch.equal(again, want)
        before = runner.num_graph_replayed
        out = runner.forward(t2, p2, prm2)
        torch.cuda.synchronize()
        assert runner.num_graph_replayed == before + 1
        assert torch.equal(out, want), (trial, float((out.float() - want.float()).abs().max()))
        restore()


def test_the_none_and_awq_steps_did_not_move():
    """a "none" and an "awq" step built before and after an fp8 step was built and run give identical logits, and the
    "none" step still holds the unquantised draw the fp8 step quantises"""
    B, n_blocks, bs = 16, 200, 5
    rng = np.random.default_rng(1)
    tokens, positions, params = _batch(rng, bs, 1, [40, 3, 77, 18, 64], B, n_blocks, 1024)

    def logits(method):
        m = _step(method, bs, n_blocks, B, seed=2, **({"group_size": 128} if method == "awq" else {}))
        _filled(m, 9)
        assert not getattr(m, "fp8") and m.weight_bits == (16 if method == "none" else 4)
        assert m.dense == (method == "none") and m.lanes_min == (0 if method == "none" else -1)
        return m.forward(tokens, positions, params, return_logits=True).clone()
    before = {m: logits(m) for m in ("none", "awq")}
    fp8 = _step("fp8", bs, n_blocks, B, seed=2, keep_checkpoint=True)
    _filled(fp8, 9)
    out = fp8.forward(tokens, positions, params, return_logits=True)
    assert torch.isfinite(out.float()).all()
    for m in ("none", "awq"):
        assert torch.equal(logits(m), before[m]), m
    # the fp8 checkpoint is the "none" checkpoint of the same seed, quantised per channel
    from scalellm_amd import kernels
    dense = _step("none", bs, n_blocks, B, seed=2, keep_checkpoint=True)
    for n in ("qkv", "o", "gate_up", "down"):
        w8, sc = kernels.quantize_fp8_weight(dense.ckpt[0][n]["weight"])
        assert torch.equal(w8.view(torch.uint8), fp8.ckpt[0][n]["weight"].view(torch.uint8)), n
        assert torch.equal(sc, fp8.ckpt[0][n]["weight_scale"]), n
    rel = float((out.float() - before["none"].float()).norm() / before["none"].float().norm())
    print(f"[fp8 e2e] logits vs the unquantised step of the same seed: relative L2 {rel:.4f} (reported, not bounded)")
