"""The dense W4A4 GEMM's SiLU * mul epilogue writing MXFP4 (slm_w4a4q_linear, include/slm_hip.h section 24) against the
unfused sequence, and LlamaDecodeStep(fuse_act_quant=True) against the unfused step: the same bits."""
import dataclasses

import numpy as np
import pytest
import torch

from tests.test_dense_step_gpu import _filled
from tests.test_model_runner_gpu import _batch

from . import w4a4_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
dtypes = pytest.mark.parametrize("bits", ref.DTYPES)
FORMS = [f for f in ref.FORMS if f[1] >= 2]
# one tile pair; three output tiles (a clamped duplicate pair under NW = 4), a partial row tile; five tiles, a K tail
SHAPES = [(1, 64, 32), (33, 192, 672), (129, 320, 1312)]


@dtypes
@pytest.mark.parametrize("side", ["T", "prequantised"])
@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("rt,nw", FORMS)
def test_codes_and_scales_equal_the_unfused_sequence(bits, rt, nw, M, N, K, side):
    from scalellm_amd import kernels
    g, dt = torch.Generator(device=DEV).manual_seed(M + K), ref.torch_dtype(bits)
    a = torch.randn(M, K, device=DEV, generator=g).to(dt)
    w, sc = kernels.quantize_mxfp4_weight(torch.randn(N, K, device=DEV, generator=g) * 0.3)
    w2, sc2 = kernels.quantize_mxfp4_weight(torch.randn(64, N // 2, device=DEV, generator=g) * 0.1)
    a_in, a_scale = (a, None) if side == "T" else kernels.quantize_mxfp4_act(a)
    qbuf = torch.full((M + 2, N // 4 + 16), 0xFF, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((M + 2, N // 64 + 3), 0xFF, dtype=torch.uint8, device=DEV)
    cq, cs = qbuf[:M, :N // 4], sbuf[:M, :N // 64]
    t, out_a, out_b = (torch.empty(M, n, dtype=dt, device=DEV) for n in (N // 2, 64, 64))
    with kernels.tuning(**ref.knobs(rt, nw, 1)):
        kernels.w4a4_linear(a_in, w, sc, t, silu_mul=True, a_scale=a_scale)
        want_q, want_s = kernels.quantize_mxfp4_act(t)
        plan = kernels.w4a4_linear_plan(a_in, w, sc, cq, silu_mul=True, a_scale=a_scale, c_scale=cs, dtype=dt)
        assert (plan.row_tiles, plan.waves, plan.split_k) == (rt, nw, 1)
        kernels.w4a4_linear(a_in, w, sc, cq, silu_mul=True, a_scale=a_scale, c_scale=cs, dtype=dt)
        kernels.w4a4_linear(t, w2, sc2, out_a)                      # the next GEMM: T side over the unfused output ...
        kernels.w4a4_linear(cq, w2, sc2, out_b, a_scale=cs)         # ... and the pre-quantised side over the fused one
    assert torch.equal(cq, want_q) and torch.equal(cs, want_s)
    qbuf[:M, :N // 4], sbuf[:M, :N // 64] = 0xFF, 0xFF
    assert (qbuf == 0xFF).all() and (sbuf == 0xFF).all()           # nothing beyond the rows' own bytes, no row >= M
    assert torch.isfinite(out_a.float()).all() and torch.equal(out_a.view(torch.int16), out_b.view(torch.int16))


def test_the_keyword_rejects_every_other_combination():
    from scalellm_amd import kernels
    a = torch.zeros(4, 64, dtype=torch.bfloat16, device=DEV)
    w, sc = torch.zeros(128, 32, dtype=torch.uint8, device=DEV), torch.full((128, 2), 127, dtype=torch.uint8, device=DEV)
    cq, cs = torch.zeros(4, 32, dtype=torch.uint8, device=DEV), torch.zeros(4, 2, dtype=torch.uint8, device=DEV)
    bad = [dict(silu_mul=False), dict(silu_mul=True, defer_reduce=True), dict(silu_mul=True, bias=a[0, :].repeat(2)),
           dict(silu_mul=True, c_scale=cs[:, :1]), dict(silu_mul=True, c=a[:, :32])]
    for kw in bad:
        with pytest.raises(kernels.SlmError):
            kernels.w4a4_linear(a, w, sc, **dict(dict(c=cq, c_scale=cs), **kw))
    aq, a_scale = kernels.quantize_mxfp4_act(a)
    with pytest.raises(kernels.SlmError):                           # pre-quantised in, codes out: the type must be named
        kernels.w4a4_linear(aq, w, sc, cq, silu_mul=True, c_scale=cs, a_scale=a_scale)


def _step(bs, n_blocks, B, **kw):
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape
    return LlamaDecodeStep(LlamaShape.tiny(), bs, n_blocks, B, quant_method="mxfp4", dtype=torch.bfloat16, device=DEV,
                           seed=1, **kw)


@pytest.mark.parametrize("bs", [1, 8])
def test_the_fused_step_equals_the_unfused_step_eager_and_replayed(bs):
    from scalellm_amd.model_runner import ModelRunner, ModelRunnerOptions
    B, max_len, n_blocks = 16, 496, 400
    plain, fused = _step(bs, n_blocks, B, act_quant="mxfp4"), _step(bs, n_blocks, B, act_quant="mxfp4", fuse_act_quant=True)
    assert fused.fuse_act_quant and not plain.fuse_act_quant and "normed_q" not in plain.buf
    restore_p, restore_f = _filled(plain, 11), _filled(fused, 11)
    runner = ModelRunner(fused, DEV, ModelRunnerOptions(block_size=B, cuda_graph_max_seq_len=max_len,
                                                        cuda_graph_batch_sizes=[bs], num_decoding_tokens=1), return_logits=True)
    runner.capture_cuda_graphs(bs)
    restore_f()
    rng = np.random.default_rng(5)
    tokens, positions, params = _batch(rng, bs, 1, [int(x) for x in rng.integers(1, 150, size=bs)], B, n_blocks, plain.shape.vocab)
    hinted = dataclasses.replace(params, kv_max_seq_len=max_len)
    want = plain.forward(tokens, positions, hinted, return_logits=True).clone()
    got = fused.forward(tokens, positions, hinted, return_logits=True).clone()
    kv_eager = [L["kv"].key_cache.clone() for L in fused.layers]
    restore_f()
    before = runner.num_graph_replayed
    replayed = runner.forward(tokens, positions, params).clone()
    torch.cuda.synchronize()
    assert runner.num_graph_replayed == before + 1
    assert torch.isfinite(want.float()).all() and torch.equal(got, want) and torch.equal(replayed, want)
    for L_p, L_f, k_e in zip(plain.layers, fused.layers, kv_eager):
        assert torch.equal(L_f["kv"].key_cache, L_p["kv"].key_cache) and torch.equal(k_e, L_p["kv"].key_cache)
        assert torch.equal(L_f["kv"].value_cache, L_p["kv"].value_cache)
    restore_p()


@pytest.mark.parametrize("kw", [dict(), dict(quant_method="mxfp4"), dict(quant_method="mxfp4", act_quant="mxfp4",
                                                                         custom_allreduce=object())])
def test_fuse_act_quant_needs_mxfp4_activations_and_no_fused_allreduce(kw):
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape
    with pytest.raises(ValueError):
        LlamaDecodeStep(LlamaShape.tiny(), 4, 8, 16, device=DEV, fuse_act_quant=True, **kw)
