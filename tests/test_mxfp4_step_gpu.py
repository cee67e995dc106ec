"""A Llama decode step over OCP MXFP4 weights (LlamaDecodeStep(quant_method="mxfp4"): the four linears are
layers.{Column,Row}ParallelMxfp4Linear over slm_mxfp4_linear) against the unquantised step loaded with the
DEQUANTISED checkpoint: the MFMA sees the same T values under the same plans, so the logits are bit-identical; graph
replay and repeatability."""
import dataclasses

import numpy as np
import pytest
import torch

from tests.test_dense_step_gpu import _filled
from tests.test_model_runner_gpu import _batch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
LINEARS = ("qkv", "o", "gate_up", "down")


def _step(quant_method, max_tokens, n_blocks, B, seed=3, **kw):
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape
    return LlamaDecodeStep(LlamaShape.tiny(), max_tokens, n_blocks, B, quant_method=quant_method, dtype=torch.bfloat16,
                           device=DEV, seed=seed, **kw)


@pytest.mark.parametrize("split", [None, 2], ids=["plan", "splitk2"])
def test_mxfp4_step_equals_the_dense_step_on_the_dequantised_checkpoint(split, tune):
    """split = 2: the tiny shape's K is too shallow for the plan to split, so the knob forces two slices: o / down /
    qkv then leave deferred slabs for the RMSNorm and the RoPE + append kernel"""
    from scalellm_amd import kernels
    from scalellm_amd.decode import hf_state_dict
    from scalellm_amd.layers import ColumnParallelMxfp4Linear, RowParallelMxfp4Linear
    B, n_blocks = 16, 200
    rng = np.random.default_rng(1)
    mx = _step("mxfp4", 64, n_blocks, B, seed=2, keep_checkpoint=True)
    s = mx.shape
    assert mx.mxfp4 and not mx.fp8 and mx.dense and mx.weight_bits == 4.25 and not mx.fold_norm and mx.lanes_min == 0
    L0 = mx.layers[0]
    assert isinstance(L0["qkv"], ColumnParallelMxfp4Linear) and isinstance(L0["down"], RowParallelMxfp4Linear)
    assert L0["gate_up"].paired and mx.buf["gate_up"] is None               # the SiLU epilogue
    qkv_n = (s.n_heads + 2 * s.n_kv_heads) * s.head_dim
    assert tuple(mx.ckpt[0]["qkv"]["weight"].shape) == (qkv_n, s.hidden // 2)
    assert tuple(mx.ckpt[1]["down"]["weight_scale"].shape) == (s.hidden, s.intermediate // 32)
    sd = hf_state_dict(mx)                                                  # *.weight (nibbles) and *.weight_scale
    assert sd["model.layers.1.self_attn.k_proj.weight"].dtype == torch.uint8
    assert tuple(sd["model.layers.1.self_attn.k_proj.weight"].shape) == (s.n_kv_heads * s.head_dim, s.hidden // 2)
    assert tuple(sd["model.layers.0.mlp.up_proj.weight_scale"].shape) == (s.intermediate, s.hidden // 32)
    # the MXFP4 checkpoint is the "none" checkpoint of the same seed, quantised; the dense twin takes it dequantised
    dense = _step("none", 64, n_blocks, B, seed=2, keep_checkpoint=True)
    for li in range(s.n_layers):
        for n in LINEARS:
            w4, sc = kernels.quantize_mxfp4_weight(dense.ckpt[li][n]["weight"])
            assert torch.equal(w4, mx.ckpt[li][n]["weight"]) and torch.equal(sc, mx.ckpt[li][n]["weight_scale"]), n
            lin = mx.layers[li][n]
            wt = kernels.dequantize_mxfp4_weight(lin.weight, lin.weight_scale, torch.bfloat16)
            assert torch.equal(wt.double(), kernels.dequantize_mxfp4_weight(lin.weight, lin.weight_scale, torch.float64))
            assert wt.shape == dense.layers[li][n].weight.shape
            dense.layers[li][n].weight = wt.contiguous()
        for n in ("in_norm", "post_norm"):
            assert torch.equal(mx.layers[li][n], dense.layers[li][n])
    assert torch.equal(mx.embed, dense.embed) and torch.equal(mx.lm_head, dense.lm_head)
    if split:
        tune(SLM_LINEAR_SPLITK=split)
    for bs, q_len, kv_lens in ((5, 1, [40, 3, 77, 18, 64]), (2, 20, [20, 33]), (40, 1, [5 + (7 * i) % 90 for i in range(40)])):
        tokens, positions, params = _batch(rng, bs, q_len, kv_lens, B, n_blocks, s.vocab)
        T = tokens.numel()
        # the same plans first: the bit-identity below follows from them
        x = torch.zeros(T, s.hidden, dtype=torch.bfloat16, device=DEV)
        for n in LINEARS:
            lm, ld = mx.layers[0][n], dense.layers[0][n]
            xin = x if lm.local_in == s.hidden else torch.zeros(T, lm.local_in, dtype=torch.bfloat16, device=DEV)
            out = torch.empty(T, lm.local_out // 2 if lm.paired else lm.local_out, dtype=torch.bfloat16, device=DEV)
            for defer in (False, True) if not lm.paired else (False,):
                pm = kernels.mxfp4_linear_plan(xin, lm.weight, lm.weight_scale, out, None, defer, lm.paired)
                pd = kernels.linear_plan(xin, ld.weight, out, None, defer, lm.paired)
                assert bytes(pm) == bytes(pd), (n, T, defer)
        restore_m, restore_d = _filled(mx, 9), _filled(dense, 9)
        got = mx.forward(tokens, positions, params, return_logits=True).clone()
        want = dense.forward(tokens, positions, params, return_logits=True).clone()
        torch.cuda.synchronize()
        assert mx.last_lanes == 1
        assert all(L0[n].deferred_splits == (split or 0) for n in ("qkv", "o", "down")) and not L0["gate_up"].deferred
        assert torch.isfinite(got.float()).all()
        assert torch.equal(got, want), (bs, q_len, float((got.float() - want.float()).abs().max()))
        for L_m, L_d in zip(mx.layers, dense.layers):                       # and the same KV was appended
            assert torch.equal(L_m["kv"].key_cache, L_d["kv"].key_cache)
        restore_m()
        restore_d()


def test_mxfp4_decode_graph_replay_and_repeat_are_bit_identical():
    from scalellm_amd.model_runner import ModelRunner, ModelRunnerOptions
    B, max_len, n_blocks, bs = 16, 496, 400, 8
    model = _step("mxfp4", bs, n_blocks, B, seed=1)
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
