"""GPU tests of the rejection sampler (csrc/rejection.hip, include/slm_hip.h section 9) against the numpy
restatement of the contract (tests/rejection_ref.py) and the reference's own cases
(tests/golden/rejection_sampler_cases.npz)."""
import os

import numpy as np
import pytest
import torch

from tests import rejection_ref as rref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rejection_sampler_cases.npz")


def _seqs_to_check(n):
    return list(range(n)) if n <= 8 else sorted({0, n // 3, (2 * n) // 3, n - 1})


def _batch(n, k, V, dtype, seed, pad=0):
    """Target logits [n, k + 1, V] (dtype), draft probs [n, k, V] fp32 near the target, draft ids: the
    draft's argmax on even rows, a random id on odd rows; mixed do_sample.  pad > 0: both tensors are
    strided views into larger buffers."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    tbuf = torch.randn(n, k + 1 + (1 if pad else 0), V + pad, device=DEV, generator=g) * 3
    target = tbuf[:, :k + 1, :V].to(dtype) if not pad else tbuf.to(dtype)[:, :k + 1, :V]
    noise = torch.randn(n, k, V, device=DEV, generator=g)
    dlog = target[:, :k].float() + noise
    dbuf = torch.empty(n, k + (1 if pad else 0), V + pad, device=DEV)
    draft = dbuf[:, :k, :V]
    draft.copy_(torch.softmax(dlog, dim=-1))
    ids = draft.argmax(-1).int()
    rnd = torch.randint(0, V, (n, k), device=DEV, generator=g, dtype=torch.int32)
    odd = (torch.arange(k, device=DEV) % 2 == 1).unsqueeze(0).expand(n, k)
    ids = torch.where(odd, rnd, ids).contiguous()
    rng = np.random.default_rng(seed)
    host = dict(do_sample=rng.random(n) < 0.7, seeds=rng.integers(0, 2**63, n, dtype=np.int64),
                positions=rng.integers(0, 1 << 20, n).astype(np.int32),
                bonus=rng.integers(0, V, n).astype(np.int32))
    dev = {key: torch.from_numpy(v).to(DEV) for key, v in host.items()}
    return target, draft, ids, host, dev


def _call(target, draft, ids, dev, mask, n_top=None):
    from scalellm_amd import kernels
    n, k = ids.shape
    out = dict(accepted_lens=torch.empty(n, dtype=torch.int32, device=DEV))
    if n_top is not None:
        out["logprobs"] = torch.empty(n, k + 1, device=DEV)
        out["top_logprobs"] = torch.empty(n, k + 1, n_top, device=DEV)
        out["top_tokens"] = torch.empty(n, k + 1, n_top, dtype=torch.int32, device=DEV)
    tok = kernels.rejection_sample(ids, draft, target, dev["bonus"], mask_out_rejected=mask,
                                   do_sample=dev["do_sample"], seeds=dev["seeds"], positions=dev["positions"], **out)
    torch.cuda.synchronize()
    return tok, out


def test_basic_fixture_of_the_reference():
    from scalellm_amd.speculative import RejectionSampler
    g = np.load(GOLDEN)
    t = {key: torch.from_numpy(g[key]).to(DEV) for key in g.files}
    tok, masked = RejectionSampler.random_sample(t["basic_draft_token_ids"], t["basic_draft_probs"],
                                                 t["basic_target_probs"], t["basic_uniform"],
                                                 t["basic_bonus_token_ids"], True)
    ref = rref.validate_seq(g["basic_draft_token_ids"][0], g["basic_draft_probs"][0], g["basic_target_probs"][0],
                            5, do_sample=True, uniform=g["basic_uniform"][0], target_is_probs=True)
    r = int(ref["tokens"][2])
    assert r in (2, 4)
    assert tok.cpu().tolist() == [[1, 2, r, 5]]
    assert masked.cpu().tolist() == [[1, 2, r, -1]]
    tok2, none = RejectionSampler.random_sample(t["basic_draft_token_ids"], t["basic_draft_probs"],
                                                t["basic_target_probs"], t["basic_uniform"],
                                                t["basic_bonus_token_ids"], False)
    assert none is None and torch.equal(tok2, tok)


@pytest.mark.parametrize("dtype", DTYPES)
def test_greedy_tokens_are_the_target_argmax_and_the_mask_stops_at_a_planted_mismatch(dtype):
    from scalellm_amd.speculative import RejectionSampler
    n, k, V = 7, 4, 32000
    target, _, _, host, dev = _batch(n, k, V, dtype, seed=1)
    am = target.float().argmax(-1).int()  # [n, k + 1]
    ids = am[:, :k].clone()
    plant = [None, 0, 1, 2, 3, None, 2]
    for s, j in enumerate(plant):
        if j is not None:
            ids[s, j] = (ids[s, j] + 1) % V
    rs = RejectionSampler(torch.zeros(n, dtype=torch.bool, device=DEV))
    out = rs.forward(ids, None, target, dev["bonus"], mask_out_rejected_tokens=False)
    want = torch.cat([am[:, :k], dev["bonus"].view(n, 1)], dim=1)
    assert torch.equal(out.next_tokens, want)
    om = rs.forward(ids, None, target, dev["bonus"], mask_out_rejected_tokens=True)
    for s, j in enumerate(plant):
        f = k if j is None else j
        exp = want[s].clone()
        exp[f + 1:] = -1
        assert torch.equal(om.next_tokens[s], exp), s
        assert int(om.accepted_lens[s]) == f + 1
    # the static form on probabilities agrees
    tp = torch.softmax(target[:, :k].float(), -1)
    tok, masked = RejectionSampler.greedy_sample(ids, tp, dev["bonus"], True)
    assert torch.equal(masked, om.next_tokens)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [50, 32000, 128256])
@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("n", [1, 7, 64, 256])
def test_sampled_and_mixed_rows_match_the_restatement(n, k, V, dtype):
    pad = 24 if (n + k) % 3 == 0 else 0  # strided target and draft rows on a third of the grid
    target, draft, ids, host, dev = _batch(n, k, V, dtype, seed=n * 1000 + k * 10 + V % 7, pad=pad)
    ta, oa = _call(target, draft, ids, dev, mask=False)
    tb, ob = _call(target, draft, ids, dev, mask=True)
    tc, oc = _call(target, draft, ids, dev, mask=True, n_top=5)
    # masked = unmasked cut after f; the G = 1 launch and the per-row launch give the same bits
    f = oa["accepted_lens"].long() - 1
    keep = torch.arange(k + 1, device=DEV).unsqueeze(0) <= f.unsqueeze(1)
    assert torch.equal(tb, torch.where(keep, ta, torch.full_like(ta, -1)))
    assert torch.equal(ob["accepted_lens"], oa["accepted_lens"]) and torch.equal(oc["accepted_lens"], oa["accepted_lens"])
    assert torch.equal(tc, tb)
    ta, fa = ta.cpu().numpy(), f.cpu().numpy()
    lp, tlp, ttok = (oc[key].cpu().numpy() for key in ("logprobs", "top_logprobs", "top_tokens"))
    near_ties = 0
    for s in _seqs_to_check(n):
        x = target[s].float().cpu().numpy()
        q = draft[s].cpu().numpy()
        ref = rref.validate_seq(ids[s].cpu().numpy(), q, x, int(host["bonus"][s]), do_sample=bool(host["do_sample"][s]),
                                seed=int(host["seeds"][s]) & (2**64 - 1), position=int(host["positions"][s]))
        flipped = None  # the first row whose decision sits within 1e-5 of the boundary
        for j in range(k):
            r, u = ref["ratios"][j], ref["us"][j]
            if r is not None and np.isfinite(r) and abs(float(u) - float(r)) <= 1e-5 * float(r):
                flipped = j
                break
        last = k if flipped is None else flipped
        for j in range(last):
            if ta[s, j] != ref["tokens"][j]:
                sc = ref["scores"][j]
                assert sc is not None, (s, j, ta[s, j], ref["tokens"][j])
                o = np.argsort(-sc.astype(np.float64), kind="stable")
                assert ta[s, j] == o[1] and sc[o[1]] >= sc[o[0]] * (1 - 1e-5), (s, j)
                near_ties += 1
        if flipped is None:
            assert fa[s] == ref["f"], s
        assert ta[s, k] == host["bonus"][s]
        lw, tw, iw = rref.logprobs_rows(x, ta[s], 5)
        np.testing.assert_allclose(lp[s], lw, rtol=1e-5, atol=2e-4, err_msg=f"seq {s}")
        np.testing.assert_array_equal(ttok[s], iw, err_msg=f"seq {s}")
        np.testing.assert_allclose(tlp[s], tw, rtol=1e-5, atol=2e-4, err_msg=f"seq {s}")
    assert near_ties <= 1


def test_distribution_of_the_output_is_the_target():
    """The reference's Random case on the device: vocab 50, one target distribution, a random draft
    distribution per row, the draft token drawn from it with slm_sample; 500k rows with distinct seeds."""
    from scalellm_amd import kernels
    n, V = 500_000, 50
    rng = np.random.default_rng(0)
    p = rng.random(V) ** 3
    p /= p.sum()
    tl = np.log(p).astype(F32)
    target = torch.from_numpy(np.stack([tl, np.zeros(V, F32)])).to(DEV).unsqueeze(0).expand(n, 2, V).contiguous()
    g = torch.Generator(device=DEV).manual_seed(1)
    dlog = torch.randn(n, V, device=DEV, generator=g) * 1.5
    seeds = torch.arange(n, dtype=torch.int64, device=DEV) * 7919 + 1
    pos = torch.full((n,), 11, dtype=torch.int32, device=DEV)
    ones = torch.ones(n, dtype=torch.bool, device=DEV)
    q = torch.empty(n, V, device=DEV)
    d = kernels.sample(dlog, do_sample=ones, seeds=seeds, positions=pos, probs=q)
    tok = kernels.rejection_sample(d.view(n, 1), q.view(n, 1, V), target, torch.zeros(n, dtype=torch.int32, device=DEV),
                                   do_sample=ones, seeds=seeds, positions=pos)
    freq = np.bincount(tok[:, 0].cpu().numpy(), minlength=V) / n
    sigma = np.sqrt(p * (1 - p) / n)
    assert np.all(np.abs(freq - p) <= 5 * sigma + 1e-12), np.max(np.abs(freq - p) / sigma)


def test_joint_distribution_of_two_rows_is_the_outer_product():
    """k = 2, vocab 8, two different target rows, no masking: the unmasked (row 0, row 1) pairs follow
    p0 x p1 -- rows that shared random numbers would correlate."""
    from scalellm_amd import kernels
    n, V, k = 400_000, 8, 2
    p0 = np.array([0.3, 0.2, 0.15, 0.12, 0.1, 0.08, 0.03, 0.02])
    p1 = np.array([0.05, 0.1, 0.25, 0.05, 0.2, 0.1, 0.15, 0.1])
    tl = np.stack([np.log(p0), np.log(p1), np.zeros(V)]).astype(F32)
    target = torch.from_numpy(tl).to(DEV).unsqueeze(0).expand(n, 3, V).contiguous()
    g = torch.Generator(device=DEV).manual_seed(2)
    dlog = torch.randn(n * k, V, device=DEV, generator=g)
    seeds = torch.arange(n, dtype=torch.int64, device=DEV) * 104729 + 3
    pos = torch.full((n,), 40, dtype=torch.int32, device=DEV)
    row_pos = (pos.view(n, 1) + torch.arange(k, device=DEV, dtype=torch.int32)).reshape(-1)
    q = torch.empty(n * k, V, device=DEV)
    d = kernels.sample(dlog, do_sample=torch.ones(n * k, dtype=torch.bool, device=DEV),
                       seeds=seeds.repeat_interleave(k), positions=row_pos, probs=q)
    tok = kernels.rejection_sample(d.view(n, k), q.view(n, k, V), target, torch.zeros(n, dtype=torch.int32, device=DEV),
                                   do_sample=torch.ones(n, dtype=torch.bool, device=DEV), seeds=seeds, positions=pos)
    t = tok.cpu().numpy()
    joint = np.bincount(t[:, 0] * V + t[:, 1], minlength=V * V) / n
    want = np.outer(p0, p1).reshape(-1)
    sigma = np.sqrt(want * (1 - want) / n)
    assert np.all(np.abs(joint - want) <= 5 * sigma), np.max(np.abs(joint - want) / sigma)


def test_edge_cases():
    from scalellm_amd import kernels
    n, k, V = 64, 4, 1000
    g = torch.Generator(device=DEV).manual_seed(4)
    probs = torch.softmax(torch.randn(n, k, V, device=DEV, generator=g) * 2, -1)
    ids = torch.multinomial(probs.view(-1, V), 1, generator=g).view(n, k).int()
    ones = torch.ones(n, dtype=torch.bool, device=DEV)
    seeds = torch.arange(n, dtype=torch.int64, device=DEV)
    bonus = torch.full((n,), 7, dtype=torch.int32, device=DEV)
    lens = torch.empty(n, dtype=torch.int32, device=DEV)
    # draft == target: every ratio is exactly 1 and u < 1
    tok = kernels.rejection_sample(ids, probs, probs, bonus, target_is_probs=True, do_sample=ones, seeds=seeds,
                                   accepted_lens=lens)
    assert torch.equal(tok[:, :k], ids) and bool((lens == k + 1).all()) and bool((tok[:, k] == 7).all())
    # an out-of-range draft id rejects (and reads nothing there)
    bad = ids.clone()
    bad[:, 1] = torch.tensor([-1, V, V + 5, 1 << 30], dtype=torch.int32, device=DEV).repeat(n // 4)
    tok = kernels.rejection_sample(bad, probs, probs, bonus, target_is_probs=True, do_sample=ones, seeds=seeds,
                                   accepted_lens=lens, mask_out_rejected=True)
    assert bool((lens == 2).all()) and bool((tok[:, 2:] == -1).all()) and bool((tok[:, 1] >= 0).all())
    assert bool((tok[:, 1] < V).all())
    # q_d == 0: p_d > 0 accepts (ratio +inf), p_d == 0 rejects (0 / 0)
    q = probs.clone()
    q[:, 0].scatter_(1, ids[:, 0:1].long(), 0.0)
    p = probs.clone()
    p[: n // 2, 0].scatter_(1, ids[: n // 2, 0:1].long(), 0.0)
    tok = kernels.rejection_sample(ids, q, p, bonus, target_is_probs=True, do_sample=ones, seeds=seeds,
                                   accepted_lens=lens, mask_out_rejected=True)
    assert bool((lens[: n // 2] == 1).all()), lens
    assert bool((tok[n // 2:, 0] == ids[n // 2:, 0]).all())
    # n_seqs == 0 is a no-op
    e = kernels.rejection_sample(torch.empty(0, k, dtype=torch.int32, device=DEV), torch.empty(0, k, V, device=DEV),
                                 torch.empty(0, k + 1, V, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV))
    assert e.shape == (0, k + 1)


def test_repeats_permutations_and_graph_replay_are_bit_identical():
    from scalellm_amd import kernels
    n, k, V = 48, 4, 50257
    target, draft, ids, host, dev = _batch(n, k, V, torch.bfloat16, seed=9)
    t1, o1 = _call(target, draft, ids, dev, mask=True, n_top=4)
    t2, o2 = _call(target, draft, ids, dev, mask=True, n_top=4)
    assert torch.equal(t1, t2) and all(torch.equal(o1[key], o2[key]) for key in o1)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(DEV)
    tp, op = _call(target[perm], draft[perm], ids[perm], {key: v[perm] for key, v in dev.items()}, mask=True, n_top=4)
    assert torch.equal(tp, t1[perm])
    for key in o1:
        assert torch.equal(op[key], o1[key][perm]), key
    # graph capture, replayed with the positions advanced in place
    pos = dev["positions"].clone()
    tok_g = torch.empty(n, k + 1, dtype=torch.int32, device=DEV)
    lens_g = torch.empty(n, dtype=torch.int32, device=DEV)
    kw = dict(mask_out_rejected=True, do_sample=dev["do_sample"], seeds=dev["seeds"], positions=pos,
              next_tokens=tok_g, accepted_lens=lens_g)
    kernels.rejection_sample(ids, draft, target, dev["bonus"], **kw)  # warm-up: sizes the workspace
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        kernels.rejection_sample(ids, draft, target, dev["bonus"], **kw)
    for step in range(3):
        pos.copy_(dev["positions"] + step)
        g.replay()
        torch.cuda.synchronize()
        te, oe = _call(target, draft, ids, dict(dev, positions=pos), mask=True)
        assert torch.equal(tok_g, te) and torch.equal(lens_g, oe["accepted_lens"]), step


def test_interleaved_sequences_are_read_in_place():
    """A [k + 1, n, V] target and a [k, n, V] draft viewed as [n, k(+1), V] (sequence stride < row stride)."""
    from scalellm_amd import kernels
    n, k, V = 16, 4, 1000
    target, draft, ids, host, dev = _batch(n, k, V, torch.bfloat16, seed=21)
    t_il = target.transpose(0, 1).contiguous().transpose(0, 1)  # [n, k + 1, V] view of a [k + 1, n, V] buffer
    d_il = draft.transpose(0, 1).contiguous().transpose(0, 1)
    assert t_il.stride(0) < t_il.stride(1) and d_il.stride(0) < d_il.stride(1)
    for mask, n_top in ((True, None), (False, None), (True, 3)):
        want, ow = _call(target.contiguous(), draft.contiguous(), ids, dev, mask=mask, n_top=n_top)
        got, og = _call(t_il, d_il, ids, dev, mask=mask, n_top=n_top)
        assert torch.equal(got, want)
        for key in ow:
            assert torch.equal(og[key], ow[key]), key
