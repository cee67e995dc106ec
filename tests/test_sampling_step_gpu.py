"""The decode step with sampling (LlamaDecodeStep.forward(..., sampling=...)): greedy parameters give
today's greedy tokens exactly, and the sampled step replays from a hipGraph bit-identically."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model(bs):
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape, make_decode_inputs
    shape = LlamaShape.tiny()
    B, kv_len = 16, 80
    tokens, positions, params, n_blocks = make_decode_inputs(bs, kv_len, B, DEV, seed=2, vocab=shape.vocab)
    model = LlamaDecodeStep(shape, bs, n_blocks, B, dtype=torch.bfloat16, device=DEV, seed=4, kv_fill="randn",
                            group_size=128)
    return model, tokens, positions, params


@pytest.mark.parametrize("bs", [1, 7, 32])
def test_greedy_parameters_reproduce_the_greedy_step(bs):
    from scalellm_amd.sampling import SamplingParameter, SamplingParameters
    model, tokens, positions, params = _model(bs)
    greedy = model.forward(tokens, positions, params).clone()
    sp = SamplingParameters.create([SamplingParameter(temperature=1.0) for _ in range(bs)], device=DEV)
    out = model.forward(tokens, positions, params, sampling=sp)
    torch.cuda.synchronize()
    assert torch.equal(out.next_tokens, greedy)
    # the reference's default temperature (0.7) scales the logits: the argmax does not move
    sp07 = SamplingParameters.create([SamplingParameter() for _ in range(bs)], device=DEV, compact=False,
                                     max_unique=4)
    out = model.forward(tokens, positions, params, sampling=sp07)
    torch.cuda.synchronize()
    assert torch.equal(out.next_tokens, greedy)


def test_sampled_step_graph_replay_equals_eager():
    from scalellm_amd.sampling import SamplingParameter, SamplingParameters
    bs = 8
    model, tokens, positions, params = _model(bs)
    greedy = model.forward(tokens, positions, params).clone()
    reqs = [SamplingParameter(temperature=0.9, top_k=20 if r % 2 else -1, top_p=0.9, do_sample=r != 3,
                              repetition_penalty=1.1, frequency_penalty=0.1, logprobs=True, top_logprobs=2,
                              seed=77 + r) for r in range(bs)]
    ids = [[int(t) for t in torch.randint(0, 1024, (6,))] for _ in range(bs)]
    sp = SamplingParameters.create(reqs, ids, device=DEV, compact=False)
    eager = model.forward(tokens, positions, params, sampling=sp)
    e_tok, e_lp = eager.next_tokens.clone(), eager.logprobs.clone()
    e_top = eager.top_tokens.clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on the capture stream
        model.forward(tokens, positions, params, sampling=sp)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = model.forward(tokens, positions, params, sampling=sp)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.next_tokens, e_tok)
        assert torch.equal(out.logprobs, e_lp) and torch.equal(out.top_tokens, e_top)
    # the sampled rows really sample: another seed moves some token (vocab 1024, temperature 0.9)
    sp2 = SamplingParameters.create([SamplingParameter(**{**r.__dict__, "seed": r.seed + 1000}) for r in reqs],
                                    ids, device=DEV, compact=False)
    sp.copy_(sp2)
    g.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out.next_tokens, e_tok)
    assert int(out.next_tokens[3]) == int(e_tok[3])  # the greedy row does not depend on the seed
    # refreshed from a COMPACT greedy batch (its neutral fields are None): nothing of the sampled batch
    # -- do_sample, top-k / top-p, penalties, penalised ids -- may survive in the tensors the graph reads
    sp.copy_(SamplingParameters.create([SamplingParameter(temperature=1.0) for _ in range(bs)], device=DEV))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.next_tokens, greedy)


@pytest.mark.parametrize("bs", [3, 128])
def test_cpp_and_python_hosts_sample_bit_identically(bs):
    """slm::LlamaForCausalLMHip::sample_step vs LlamaDecodeStep.forward(sampling=...) on the same 2-layer
    AWQ weights, KV caches and parameters: tokens, logprobs and top logprobs bit-identical (bs 128: both
    hosts run the step as two lanes)."""
    import numpy as np
    from scalellm_amd import cpp_host
    from scalellm_amd.sampling import SamplingParameter, SamplingParameters
    from tests.test_cpp_host_step_gpu import _step
    from tests.test_model_runner_gpu import _batch
    B, n_blocks, max_tokens = 16, 3000, 200
    step, shape = _step("awq", max_tokens, n_blocks, B)
    step.reserve_workspaces(max_tokens, 512)
    cpp = cpp_host.from_decode_step(step, B, max_tokens, lanes=64)
    rng = np.random.default_rng(bs)
    snap = [(L["kv"].key_cache.clone(), L["kv"].value_cache.clone()) for L in step.layers]

    def restore():
        for L, (k0, v0) in zip(step.layers, snap):
            L["kv"].key_cache.copy_(k0)
            L["kv"].value_cache.copy_(v0)
    tokens, positions, params = _batch(rng, bs, 1, [int(x) for x in rng.integers(1, 300, size=bs)], B, n_blocks,
                                       shape.vocab)
    reqs = [SamplingParameter(temperature=0.8, top_k=[-1, 40, 5][r % 3], top_p=[1.0, 0.9][r % 2],
                              repetition_penalty=1.2, frequency_penalty=0.3, presence_penalty=0.2,
                              do_sample=r % 4 != 0, logprobs=True, top_logprobs=3, seed=31 * r + 1) for r in range(bs)]
    ids = [[int(t) for t in rng.choice(shape.vocab, 8, replace=False)] for _ in range(bs)]
    cnt = [[int(c) for c in rng.integers(0, 3, 8)] for _ in range(bs)]
    sp = SamplingParameters.create(reqs, ids, cnt, device=DEV)
    want = step.forward(tokens, positions, params, sampling=sp)
    w_tok, w_lp, w_top, w_tlp = (want.next_tokens.clone(), want.logprobs.clone(), want.top_tokens.clone(),
                                 want.top_logprobs.clone())
    lanes_py = step.last_lanes
    restore()
    got = cpp.sample_step(tokens, positions, cpp_host.cpp_params(params), cpp_host.cpp_sampling_params(sp))
    torch.cuda.synchronize()
    assert cpp.last_lanes() == lanes_py == (2 if bs >= 64 else 1)
    assert torch.equal(got.next_tokens, w_tok)
    assert torch.equal(got.logprobs, w_lp)
    assert torch.equal(got.top_tokens, w_top) and torch.equal(got.top_logprobs, w_tlp)
    restore()
