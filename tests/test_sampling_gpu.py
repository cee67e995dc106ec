"""GPU tests of the fused logits processing + sampling kernel (csrc/sampling.hip, include/slm_hip.h
section 8) against the numpy restatement of the contract (tests/sampling_ref.py)."""
import numpy as np
import pytest
import torch

from tests import sampling_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
DTYPES = [torch.float16, torch.bfloat16, torch.float32]


def _batch(n, V, dtype, seed, max_unique=64, sample_frac=0.6):
    """Random logits and mixed per-row parameters (every knob on some rows, neutral on others)."""
    rng = np.random.default_rng(seed)
    logits = torch.from_numpy((rng.standard_normal((n, V)) * 3).astype(F32)).to(dtype).to(DEV)
    ids = np.zeros((n, max_unique), np.int64)
    counts = np.zeros((n, max_unique), np.int32)
    lens = rng.integers(0, max_unique + 1, n).astype(np.int32)
    for r in range(n):
        ids[r, :lens[r]] = rng.choice(V, lens[r], replace=False)
        counts[r, :lens[r]] = rng.integers(0, 4, lens[r])
    p = dict(
        frequency_penalties=rng.choice([0.0, 0.1, 0.5], n).astype(F32),
        presence_penalties=rng.choice([0.0, 0.2, 1.0], n).astype(F32),
        repetition_penalties=rng.choice([1.0, 1.1, 1.3], n).astype(F32),
        temperatures=rng.choice([0.0, 0.5, 0.7, 1.0, 1.3], n).astype(F32),
        top_k=rng.choice([-1, 0, 1, 5, 50, V], n).astype(np.int64),
        top_p=rng.choice([1.0, 0.95, 0.9, 0.5, 0.0], n).astype(F32),
        do_sample=rng.random(n) < sample_frac,
        seeds=rng.integers(0, 2**63, n, dtype=np.int64),
        positions=rng.integers(0, 1 << 20, n).astype(np.int32),
    )
    host = dict(p, unique_token_ids=ids, unique_token_counts=counts, unique_token_lens=lens)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in host.items()}
    return logits, host, dev


def _oracle_process(x32, host, r, filters=True):
    return ref.process_row(
        x32[r], freq=host["frequency_penalties"][r], pres=host["presence_penalties"][r],
        rep=host["repetition_penalties"][r], temp=host["temperatures"][r],
        top_k=host["top_k"][r] if filters else None, top_p=host["top_p"][r] if filters else None,
        ids=host["unique_token_ids"][r], counts=host["unique_token_counts"][r],
        n_ids=int(host["unique_token_lens"][r]))


def _round(x32, dtype):
    return torch.from_numpy(x32).to(dtype).float().numpy()


def _rows_to_check(n):
    return list(range(n)) if n <= 8 else sorted(set(range(0, n, max(1, n // 10))) | {n - 1})


def _run(logits, dev, n_top=0, want_probs=False):
    from scalellm_amd import kernels
    n, V = logits.shape
    out = dict(processed=torch.empty_like(logits), logprobs=torch.empty(n, device=DEV))
    if n_top:
        out["top_logprobs"] = torch.empty(n, n_top, device=DEV)
        out["top_tokens"] = torch.empty(n, n_top, dtype=torch.int32, device=DEV)
    if want_probs:
        out["probs"] = torch.empty(n, V, device=DEV)
    tok = kernels.sample(logits, **dev, **out)
    torch.cuda.synchronize()
    return tok, out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [1024, 50257, 128256])
@pytest.mark.parametrize("n", [1, 7, 32, 256])
def test_processed_tokens_and_logprobs_match_the_oracle(dtype, V, n):
    logits, host, dev = _batch(n, V, dtype, seed=V + n)
    tok, out = _run(logits, dev, n_top=5)
    x32 = logits.float().cpu().numpy()
    proc = out["processed"].float().cpu().numpy()
    tok = tok.cpu().numpy()
    lp, tlp = out["logprobs"].cpu().numpy(), out["top_logprobs"].cpu().numpy()
    ttok = out["top_tokens"].cpu().numpy()
    near_ties = 0
    for r in _rows_to_check(n):
        want, excl = _oracle_process(x32, host, r)
        got = proc[r]
        fin_w, fin_g = np.isfinite(want), np.isfinite(got)
        diff = fin_w != fin_g
        if diff.any():  # only at a top-p boundary the oracle itself cannot place to 1e-5
            assert excl is not None, (r, np.nonzero(diff)[0][:5])
            assert np.all(np.abs(excl[diff] - float(F32(host["top_p"][r]))) < 1e-5), r
            # the row goes on with the kernel's own kept set over the oracle's values: value bits, token, logprob
            # and top-n are checked against the set the kernel chose (tests/test_vocab_exact_gpu.py pins the set
            # itself where the boundary can be placed exactly)
            vals, _ = _oracle_process(x32, host, r, filters=False)
            want = np.where(fin_g, vals, F32(-np.inf)).astype(F32)
            fin_w = fin_g
        np.testing.assert_array_equal(got[fin_g], _round(want[fin_w], dtype), err_msg=f"row {r}")
        # tokens: greedy rows exactly, sampled rows by the oracle's race over the same fp32 values
        if host["do_sample"][r]:
            s = ref.race_scores(want, int(host["seeds"][r]) & (2**64 - 1), int(host["positions"][r]))
            o = np.argsort(-s.astype(np.float64), kind="stable")
            if tok[r] != o[0]:
                assert tok[r] == o[1] and s[o[1]] >= s[o[0]] * (1 - 1e-5), (r, tok[r], o[:2])
                near_ties += 1
        else:
            assert tok[r] == int(np.argmax(want)), r
        lp_w, top_v, top_i = ref.logprobs_row(want, int(tok[r]), 5)
        assert lp[r] == pytest.approx(lp_w, abs=2e-4, rel=1e-5)
        np.testing.assert_array_equal(ttok[r], top_i)
        np.testing.assert_allclose(tlp[r], top_v, rtol=1e-5, atol=2e-4)
    assert near_ties <= 1


def test_rng_bits_are_pinned_on_equal_logits():
    """All logits equal, no filtering: the race is argmax of the uniform stream -- the Philox words."""
    from scalellm_amd import kernels
    n, V = 64, 1024
    rng = np.random.default_rng(3)
    seeds = rng.integers(0, 2**63, n, dtype=np.int64)
    pos = rng.integers(0, 1 << 30, n).astype(np.int32)
    tok = kernels.sample(torch.zeros(n, V, dtype=torch.bfloat16, device=DEV),
                         do_sample=torch.ones(n, dtype=torch.bool, device=DEV),
                         seeds=torch.from_numpy(seeds).to(DEV), positions=torch.from_numpy(pos).to(DEV))
    tok = tok.cpu().numpy()
    for r in range(n):
        u = ref.uniform24(ref.philox_words(int(seeds[r]), int(pos[r]), np.arange(V)))
        assert tok[r] == int(np.argmax(u)), r


def test_repeats_permutations_and_graph_replay_are_bit_identical():
    n, V = 48, 50257
    logits, host, dev = _batch(n, V, torch.bfloat16, seed=11)
    t1, o1 = _run(logits, dev, n_top=4, want_probs=True)
    t2, o2 = _run(logits, dev, n_top=4, want_probs=True)
    assert torch.equal(t1, t2)
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(DEV)
    tp, op = _run(logits[perm].contiguous(), {k: v[perm].contiguous() for k, v in dev.items()}, n_top=4,
                  want_probs=True)
    assert torch.equal(tp, t1[perm])
    for k in o1:
        assert torch.equal(op[k], o1[k][perm]), k
    # graph capture, replayed three times with the positions advanced in place
    from scalellm_amd import kernels
    pos = dev["positions"].clone()
    dev_g = dict(dev, positions=pos)
    tok_g = torch.empty(n, dtype=torch.int32, device=DEV)
    lp_g = torch.empty(n, device=DEV)
    kernels.sample(logits, next_tokens=tok_g, logprobs=lp_g, **dev_g)  # warm-up (workspace)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        kernels.sample(logits, next_tokens=tok_g, logprobs=lp_g, **dev_g)
    for step in range(3):
        pos.copy_(dev["positions"] + step)
        g.replay()
        torch.cuda.synchronize()
        te = kernels.sample(logits, logprobs=(lp_e := torch.empty(n, device=DEV)), **dict(dev, positions=pos))
        torch.cuda.synchronize()
        assert torch.equal(tok_g, te) and torch.equal(lp_g, lp_e), step


def test_sampled_distribution():
    """vocab 8, 20000 rows with distinct seeds: each token's frequency within 5 sigma of its probability
    after top-k / top-p (and exactly zero for the filtered ones)."""
    from scalellm_amd import kernels
    n, V = 20000, 8
    base = np.log(np.array([0.3, 0.2, 0.15, 0.12, 0.1, 0.08, 0.03, 0.02])).astype(F32)
    logits = torch.from_numpy(np.tile(base, (n, 1))).to(DEV)
    for top_k, top_p in ((-1, 1.0), (5, 1.0), (-1, 0.7), (6, 0.8)):
        want, _ = ref.process_row(base, top_k=top_k, top_p=top_p)
        p = np.exp(want.astype(np.float64) - want.max())
        p /= p.sum()
        tok = kernels.sample(logits, do_sample=torch.ones(n, dtype=torch.bool, device=DEV),
                             seeds=torch.arange(n, dtype=torch.int64, device=DEV) * 7919 + 1,
                             positions=torch.full((n,), 5, dtype=torch.int32, device=DEV),
                             top_k=torch.full((n,), top_k, dtype=torch.int64, device=DEV),
                             top_p=torch.full((n,), top_p, device=DEV))
        freq = np.bincount(tok.cpu().numpy(), minlength=V) / n
        sigma = np.sqrt(p * (1 - p) / n)
        assert np.all(np.abs(freq - p) <= 5 * sigma + 1e-12), (top_k, top_p, freq, p)


@pytest.mark.parametrize("dtype", DTYPES)
def test_drop_in_penalty_functions_round_once_per_call(dtype):
    """kernels.apply_*_penalty: the reference kernels' signatures, in place, rounded to the dtype at the
    end of each call (penalty_kernels.cu)."""
    from scalellm_amd import kernels
    n, V = 9, 50257
    logits, host, dev = _batch(n, V, dtype, seed=5)
    x = logits.clone()
    kernels.apply_frequency_presence_penalty(x, dev["unique_token_ids"], dev["unique_token_counts"],
                                             dev["unique_token_lens"], dev["frequency_penalties"][:, None],
                                             dev["presence_penalties"][:, None])
    x1 = x.float().cpu().numpy()
    kernels.apply_repetition_penalty(x, dev["unique_token_ids"], dev["unique_token_lens"],
                                     dev["repetition_penalties"])
    x2 = x.float().cpu().numpy()
    kernels.apply_temperature_penalty(x, dev["temperatures"])
    x3 = x.float().cpu().numpy()
    x0 = logits.float().cpu().numpy()
    for r in range(n):
        k = dict(ids=host["unique_token_ids"][r], counts=host["unique_token_counts"][r],
                 n_ids=int(host["unique_token_lens"][r]))
        w1, _ = ref.process_row(x0[r], freq=host["frequency_penalties"][r], pres=host["presence_penalties"][r], **k)
        np.testing.assert_array_equal(x1[r], _round(w1, dtype))
        w2, _ = ref.process_row(x1[r], rep=host["repetition_penalties"][r], **k)
        np.testing.assert_array_equal(x2[r], _round(w2, dtype))
        w3, _ = ref.process_row(x2[r], temp=host["temperatures"][r])
        np.testing.assert_array_equal(x3[r], _round(w3, dtype))


def test_python_api_matches_the_fused_kernel():
    """LogitsProcessor.create + Sampler (the reference's two objects) == sample_logits (one launch)."""
    from scalellm_amd.sampling import LogitsProcessor, Sampler, SamplingParameter, SamplingParameters, sample_logits
    n, V = 16, 4096
    rng = np.random.default_rng(9)
    reqs = [SamplingParameter(frequency_penalty=0.2, presence_penalty=0.1, repetition_penalty=1.2,
                              temperature=0.8, top_k=40, top_p=0.9, do_sample=bool(r % 3), logprobs=True,
                              top_logprobs=3, seed=1000 + r) for r in range(n)]
    ids = [list(rng.choice(V, 10, replace=False)) for _ in range(n)]
    cnt = [list(rng.integers(1, 4, 10)) for _ in range(n)]
    params = SamplingParameters.create(reqs, ids, cnt, device=DEV)
    logits = torch.randn(n, V, device=DEV, dtype=torch.float32)  # fp32: nothing rounds between the two launches
    pos = torch.arange(n, dtype=torch.int32, device=DEV)
    fused = sample_logits(logits, params, pos)
    proc = LogitsProcessor.create(params)(logits.clone(), params.unique_token_ids, params.unique_token_counts,
                                          params.unique_token_ids_lens)
    out = Sampler(params.do_sample, True, 3, seeds=params.seeds, positions=pos).forward(proc)
    torch.cuda.synchronize()
    assert torch.equal(fused.next_tokens, out.next_tokens)
    assert torch.equal(fused.logprobs, out.logprobs)
    assert torch.equal(fused.top_tokens, out.top_tokens) and torch.equal(fused.top_logprobs, out.top_logprobs)
    assert out.probs.shape == (n, V) and torch.allclose(out.probs.sum(-1), torch.ones(n, device=DEV), atol=1e-4)
    assert bool((out.probs[proc == -float("inf")] == 0).all())
