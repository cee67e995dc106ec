"""The verify step of speculative decoding on both hosts (LlamaDecodeStep.verify and
slm::LlamaForCausalLMHip::verify_step) over a tiny 2-layer AWQ Llama: k + 1 rows per sequence, processed in
place, bonus token from the last processed row, drafts validated by the rejection kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, N_BLOCKS, MAX_TOKENS, KV_LEN = 16, 3000, 200, 80


@pytest.fixture(scope="module")
def hosts():
    from scalellm_amd import cpp_host
    from tests.test_cpp_host_step_gpu import _step
    step, shape = _step("awq", MAX_TOKENS, N_BLOCKS, B)
    step.reserve_workspaces(MAX_TOKENS, 512)
    cpp = cpp_host.from_decode_step(step, B, MAX_TOKENS)
    return step, shape, cpp


def _inputs(n, k, vocab, seed):
    from scalellm_amd.decode import make_decode_inputs
    tokens, positions, params, n_blocks = make_decode_inputs(n, KV_LEN, B, DEV, seed=seed, q_len=k + 1, vocab=vocab)
    assert n_blocks <= N_BLOCKS
    return tokens, positions, params


def _cpp(cpp, tokens, positions, params, drafts, probs, sp, mask=True):
    from scalellm_amd import cpp_host
    return cpp.verify_step(tokens, positions, cpp_host.cpp_params(params), drafts, probs,
                           cpp_host.cpp_sampling_params(sp), mask)


def test_greedy_argmax_chain_is_accepted_and_a_planted_draft_rejects(hosts):
    from scalellm_amd.sampling import SamplingParameter, SamplingParameters
    step, shape, cpp = hosts
    n, k, V = 5, 4, shape.vocab
    tokens, positions, params = _inputs(n, k, V, seed=1)
    sp = SamplingParameters.create([SamplingParameter(temperature=1.0) for _ in range(n * (k + 1))], device=DEV)
    rows_in = tokens.view(n, k + 1)
    drafts = torch.zeros(n, k, dtype=torch.int32, device=DEV)
    for j in range(k):  # row j's logits depend on the drafts before it: build the chain one row per step
        rows_in[:, 1:] = drafts
        step.verify(tokens, positions, params, drafts, None, sp)
        drafts[:, j] = step.verify_logits.view(n, k + 1, V)[:, j].argmax(-1).int()
    rows_in[:, 1:] = drafts
    out = step.verify(tokens, positions, params, drafts, None, sp)
    torch.cuda.synchronize()
    argmax = step.verify_logits.view(n, k + 1, V).argmax(-1).int()
    assert torch.equal(argmax[:, :k], drafts)
    assert bool((out.accepted_lens == k + 1).all())
    assert torch.equal(out.next_tokens, argmax)  # the drafts, then the greedy bonus
    got = _cpp(cpp, tokens, positions, params, drafts, None, sp)
    torch.cuda.synchronize()
    assert torch.equal(got.next_tokens, out.next_tokens) and torch.equal(got.accepted_lens, out.accepted_lens)
    # a wrong draft at row j_s: f = j_s, and row j_s holds the target argmax
    plant = torch.arange(n, device=DEV) % k
    bad = drafts.clone()
    bad[torch.arange(n, device=DEV), plant] = (drafts[torch.arange(n, device=DEV), plant] + 1) % V
    rows_in[:, 1:] = bad
    for run in (lambda: step.verify(tokens, positions, params, bad, None, sp),
                lambda: _cpp(cpp, tokens, positions, params, bad, None, sp)):
        o = run()
        torch.cuda.synchronize()
        for s in range(n):
            j = int(plant[s])
            assert int(o.accepted_lens[s]) == j + 1, s
            assert torch.equal(o.next_tokens[s, :j + 1], drafts[s, :j + 1]), s  # row j: the argmax = chain draft
            assert bool((o.next_tokens[s, j + 1:] == -1).all()), s


def _sampled_params(n, k, vocab, seed, logprobs=True):
    from scalellm_amd.sampling import SamplingParameter, SamplingParameters
    rng = np.random.default_rng(seed)
    T = n * (k + 1)
    reqs, ids, cnt = [], [], []
    for s in range(n):
        base = dict(temperature=0.8, top_k=[-1, 40, 5][s % 3], top_p=[1.0, 0.9][s % 2], repetition_penalty=1.2,
                    frequency_penalty=0.3, presence_penalty=0.2, do_sample=s % 4 != 0, logprobs=logprobs,
                    top_logprobs=3 if logprobs else 0, seed=31 * s + 1)
        seq_ids = [int(t) for t in rng.choice(vocab, 8, replace=False)]
        for j in range(k + 1):  # one parameter row per verify row; the penalty counts grow along the drafts
            reqs.append(SamplingParameter(**base))
            ids.append(seq_ids)
            cnt.append([int(c) + j for c in rng.integers(0, 3, 8)])
    return SamplingParameters.create(reqs, ids, cnt, device=DEV), T


def _drafts(n, k, vocab, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    probs = torch.softmax(torch.randn(n, k, vocab, device=DEV, generator=g) * 2, -1)
    ids = torch.multinomial(probs.view(-1, vocab), 1, generator=g).view(n, k).int()
    return ids, probs


def test_processed_rows_equal_slm_logits_process(hosts):
    from scalellm_amd import kernels
    step, shape, cpp = hosts
    n, k, V = 6, 3, shape.vocab
    tokens, positions, params = _inputs(n, k, V, seed=2)
    sp, T = _sampled_params(n, k, V, seed=2)
    ids, probs = _drafts(n, k, V, seed=2)
    tokens.view(n, k + 1)[:, 1:] = ids
    step.verify(tokens, positions, params, ids, probs, sp)
    raw = step.last_hidden @ step.lm_head  # the same GEMM on the same rows
    p = sp.narrow(T)
    want = kernels.logits_process(raw.clone(), unique_token_ids=p.unique_token_ids,
                                  unique_token_counts=p.unique_token_counts, unique_token_lens=p.unique_token_ids_lens,
                                  **p.processing_kwargs())
    torch.cuda.synchronize()
    assert not torch.equal(raw, want)  # the parameters do process the rows
    assert torch.equal(step.verify_logits, want)
    _cpp(cpp, tokens, positions, params, ids, probs, sp)
    torch.cuda.synchronize()
    assert torch.equal(cpp.last_verify_logits(), want)


@pytest.mark.parametrize("mask", [True, False])
def test_sampled_verify_steps_are_bit_identical_on_both_hosts(hosts, mask):
    step, shape, cpp = hosts
    n, k, V = 12, 4, shape.vocab
    tokens, positions, params = _inputs(n, k, V, seed=3)
    sp, _ = _sampled_params(n, k, V, seed=3)
    ids, probs = _drafts(n, k, V, seed=3)
    tokens.view(n, k + 1)[:, 1:] = ids
    want = step.verify(tokens, positions, params, ids, probs, sp, mask_out_rejected_tokens=mask)
    w = {name: getattr(want, name).clone() for name in ("next_tokens", "accepted_lens", "logprobs", "top_logprobs",
                                                        "top_tokens")}
    got = _cpp(cpp, tokens, positions, params, ids, probs, sp, mask)
    torch.cuda.synchronize()
    for name, t in w.items():
        assert torch.equal(getattr(got, name), t), name
    assert w["next_tokens"].shape == (n, k + 1) and w["top_tokens"].shape == (n, k + 1, 3)


def test_captured_verify_step_replays_bit_identically(hosts):
    step, shape, cpp = hosts
    n, k, V = 8, 4, shape.vocab
    tokens, positions, params = _inputs(n, k, V, seed=4)
    sp, _ = _sampled_params(n, k, V, seed=4)
    ids, probs = _drafts(n, k, V, seed=4)
    tokens.view(n, k + 1)[:, 1:] = ids
    eager = step.verify(tokens, positions, params, ids, probs, sp)
    e = {name: getattr(eager, name).clone() for name in ("next_tokens", "accepted_lens", "logprobs", "top_tokens")}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on the capture stream
        step.verify(tokens, positions, params, ids, probs, sp)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step.verify(tokens, positions, params, ids, probs, sp)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        for name, t in e.items():
            assert torch.equal(getattr(out, name), t), name
