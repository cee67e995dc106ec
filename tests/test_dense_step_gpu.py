"""A Llama decode step over UNQUANTISED weights (LlamaDecodeStep(quant_method="none"): the four linears are
layers.{Column,Row}ParallelLinear over slm_linear) against the oracle-composed fp32 forward and its bf16-storage
twin, with the tolerances tests/test_e2e_gpu.py holds the 4-bit model to; graph replay, repeatability, the two-lane
form on request, and a guard that the int4 step did not move."""
import dataclasses

import numpy as np
import pytest
import torch

from tests.e2e_common import OracleLlama, Sequences, check_logits
from tests.test_model_runner_gpu import _batch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None


def _params(inp):
    from scalellm_amd.layers import InputParameters
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return (t(inp["tokens"]), t(inp["positions"]),
            InputParameters(q_cu_seq_lens=t(inp["q_cu"]), kv_cu_seq_lens=t(inp["kv_cu"]),
                            new_cache_slots=t(inp["slots"]), block_tables=t(inp["table"]),
                            cu_block_lens=t(inp["bcu"]), q_max_seq_len=inp["max_q"],
                            kv_max_seq_len=inp["max_kv"]))


def _oracle_twin(model, storage=None):
    """The same model rebuilt on the CPU from the kept checkpoint: weight [N, K] -> the oracle's dense [K, N] fp32"""
    s = model.shape
    f = lambda t: t.float().cpu().numpy()  # noqa: E731
    layers = []
    for li, ck in enumerate(model.ckpt):
        W = {n: np.ascontiguousarray(f(ck[n]["weight"]).T) for n in ("qkv", "o", "gate_up", "down")}
        W["in_norm"], W["post_norm"] = f(model.layers[li]["in_norm"]), f(model.layers[li]["post_norm"])
        layers.append(W)
    D = s.head_dim
    inv_freq = (1.0 / (s.rope_theta ** (np.arange(0, D, 2, dtype=np.float32) / D))).astype(np.float32)
    return OracleLlama(layers, f(model.final_norm), f(model.embed), f(model.lm_head), s.n_heads, s.n_kv_heads, D,
                       s.rms_eps, inv_freq, model.block_size, model.layers[0]["kv"].key_cache.size(0), storage=storage)


def _dense(max_tokens, n_blocks, B, seed=3, **kw):
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape
    return LlamaDecodeStep(LlamaShape.tiny(), max_tokens, n_blocks, B, quant_method="none", dtype=torch.bfloat16,
                           device=DEV, seed=seed, **kw)


@pytest.mark.parametrize("split", [None, 2], ids=["plan", "splitk2"])
def test_dense_step_prefill_chunk_and_decode_match_the_oracle(split, tune):
    """split = 2: the tiny shape's K (256 / 512) is too shallow for the plan to split, so the knob forces two slices:
    o / down / qkv then leave deferred slabs for the RMSNorm and the RoPE + append kernel in every step"""
    from scalellm_amd.decode import hf_state_dict
    from scalellm_amd.layers import ColumnParallelLinear, RowParallelLinear
    B, n_seq = 16, 40
    prompt_lens = [30, 45, 20] + [3 + (7 * i) % 11 for i in range(n_seq - 3)]
    seqs = Sequences(prompt_lens, 4, B, 1024, seed=7)
    rest = [0] * (n_seq - 3)
    steps = [("prefill of 70 tokens over 3 sequences", [30, 20, 20] + rest),
             ("chunked continuation beside two decode rows", [1, 25, 1] + rest),
             ("decode at T = 3", [1, 1, 1] + rest),
             ("prefill of the other 37 sequences", [0, 0, 0] + prompt_lens[3:]),
             ("decode at T = 40", [1] * n_seq)]
    model = _dense(sum(prompt_lens) + 8, seqs.n_blocks, B, keep_checkpoint=True)
    s = model.shape
    assert model.dense and not model.fold_norm and model.lanes_min == 0     # auto: one lane for dense weights
    L0 = model.layers[0]
    assert isinstance(L0["qkv"], ColumnParallelLinear) and isinstance(L0["down"], RowParallelLinear)
    assert L0["gate_up"].paired and model.buf["gate_up"] is None            # the SiLU epilogue
    assert tuple(model.ckpt[0]["qkv"]["weight"].shape) == ((s.n_heads + 2 * s.n_kv_heads) * s.head_dim, s.hidden)
    assert tuple(model.ckpt[1]["down"]["weight"].shape) == (s.hidden, s.intermediate)
    sd = hf_state_dict(model)                                               # plain *.weight tensors [out, in]
    assert tuple(sd["model.layers.1.self_attn.k_proj.weight"].shape) == (s.n_kv_heads * s.head_dim, s.hidden)
    assert tuple(sd["model.layers.0.mlp.up_proj.weight"].shape) == (s.intermediate, s.hidden)
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
        a, n, rel = check_logits(got, ref_model.forward(inp), 3e-2, f"dense, {what}: vs fp32 oracle")
        _, _, rel_t = check_logits(got, twin_model.forward(inp), 1.5e-2, f"dense, {what}: vs bf16-storage twin")
        agree, total = agree + a, total + n
        rels.append((round(rel, 5), round(rel_t, 5)))
        seqs.advance(new_lens)
        seqs.feed(inp, got.argmax(-1))
    print(f"[dense e2e] per-step relative L2 error (vs fp32 oracle, vs bf16-storage twin): {rels}; "
          f"greedy ids equal on {agree}/{total} rows")
    assert model.defer_splitk


def _filled(model, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    for L in model.layers:
        L["kv"].key_cache.normal_(generator=g)
        L["kv"].value_cache.normal_(generator=g)
    snap = [(L["kv"].key_cache.clone(), L["kv"].value_cache.clone()) for L in model.layers]

    def restore():
        for L, (k0, v0) in zip(model.layers, snap):
            L["kv"].key_cache.copy_(k0)
            L["kv"].value_cache.copy_(v0)
    return restore


def test_dense_decode_graph_replay_and_repeat_are_bit_identical():
    from scalellm_amd.model_runner import ModelRunner, ModelRunnerOptions
    B, max_len, n_blocks, bs = 16, 496, 400, 8
    model = _dense(bs, n_blocks, B, seed=1)
    restore = _filled(model, 11)
    rng = np.random.default_rng(5)
    opts = ModelRunnerOptions(block_size=B, cuda_graph_max_seq_len=max_len, cuda_graph_batch_sizes=[bs],
                              num_decoding_tokens=1)
    runner = ModelRunner(model, DEV, opts, return_logits=True)
    runner.capture_cuda_graphs(bs)
    restore()
    for trial in range(3):                                   # the same graph over other (advanced) lengths
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


def test_dense_two_lane_step_on_request_matches_the_one_lane_step(monkeypatch):
    B, n_blocks, bs = 16, 64 * 32, 64
    monkeypatch.setenv("SLM_DECODE_LANES", "64")             # an explicit request is honoured (auto: one lane)
    model = _dense(bs, n_blocks, B, seed=3)
    assert model.lanes_min == 64
    restore = _filled(model, 103)
    rng = np.random.default_rng(bs)
    kv = [int(x) for x in rng.integers(1, 450, size=bs)]
    tokens, positions, params = _batch(rng, bs, 1, kv, B, n_blocks, model.shape.vocab)
    model.reserve_workspaces(bs, 496)
    got = model.forward(tokens, positions, params, return_logits=True).float().clone()
    torch.cuda.synchronize()
    assert model.last_lanes == 2
    restore()
    model.lanes_min = 0
    whole = model.forward(tokens, positions, params, return_logits=True).float().clone()
    assert model.last_lanes == 1
    # (tests/test_decode_lanes_gpu.py: other row counts => other GEMM plans; the logits agree to rounding)
    rel = float((got - whole).norm() / whole.norm())
    assert rel <= 2e-2, rel


def test_the_int4_step_did_not_move():
    """an "awq" step built before and after a dense step was built and run gives identical logits"""
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape
    B, n_blocks, bs = 16, 200, 5
    rng = np.random.default_rng(1)
    tokens, positions, params = _batch(rng, bs, 1, [40, 3, 77, 18, 64], B, n_blocks, 1024)

    def awq_logits():
        m = LlamaDecodeStep(LlamaShape.tiny(), bs, n_blocks, B, quant_method="awq", group_size=128,
                            dtype=torch.bfloat16, device=DEV, seed=2)
        _filled(m, 9)
        assert not m.dense and m.weight_bits == 4 and m.lanes_min == -1
        return m.forward(tokens, positions, params, return_logits=True).clone()
    before = awq_logits()
    dense = _dense(bs, n_blocks, B, seed=2)
    _filled(dense, 9)
    out = dense.forward(tokens, positions, params, return_logits=True)
    assert torch.isfinite(out.float()).all()
    assert torch.equal(awq_logits(), before)
