"""numpy oracle of the mixture-of-experts contract (include/slm_hip.h section 10): routing, block alignment,
the sum over a token's experts and the selection margin the GPU tests use for the sigmoid routing.
Everything here is float64 unless stated; orderings are stable by index (the lower expert id first)."""
import numpy as np


def _stable_desc(v):
    """indices of v in descending order, equal values in ascending index order (-0 == +0)"""
    return np.argsort(-np.asarray(v), kind="stable")


def topk_softmax(logits, k, renormalize=False):
    """logits [T, E] -> (weights [T, k] float64, indices [T, k] int32).  Selection on the logits as given
    (fp32 logits are compared as fp32 values: the widening is exact)."""
    x = np.asarray(logits)
    T, _ = x.shape
    idx = np.argsort(-x, axis=1, kind="stable")[:, :k].astype(np.int32).reshape(T, k)
    x64 = x.astype(np.float64)
    p = np.exp(x64 - x64.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    w = np.take_along_axis(p, idx.astype(np.int64), axis=1)
    if renormalize:
        w = w / w.sum(axis=1, keepdims=True)
    return w, idx


def grouped_topk_sigmoid(logits, bias, n_groups, topk_group, k, scaling, with_margin=False):
    """grouped_topk_sigmoid_ref of the reference's test, in float64, with the tie rule made explicit.
    with_margin: also returns, per token, the smallest gap that decides the result -- between the last kept and
    the first dropped group, and between adjacent candidates among the first k + 1 of the kept experts."""
    x = np.asarray(logits, np.float64)
    b = np.asarray(bias, np.float64)
    T, E = x.shape
    gsz = E // n_groups
    s = 1.0 / (1.0 + np.exp(-x))
    c = s + b[None, :]
    W = np.zeros((T, k))
    I = np.zeros((T, k), np.int32)
    margin = np.full(T, np.inf)
    for t in range(T):
        cg = c[t].reshape(n_groups, gsz)
        top2 = -np.sort(-cg, axis=1)[:, :2]
        gscore = top2.sum(axis=1)
        gorder = _stable_desc(gscore)
        keep = np.zeros(n_groups, bool)
        keep[gorder[:topk_group]] = True
        if topk_group < n_groups:
            margin[t] = min(margin[t], gscore[gorder[topk_group - 1]] - gscore[gorder[topk_group]])
        masked = np.where(np.repeat(keep, gsz), c[t], -np.inf)
        order = _stable_desc(masked)
        sel = order[:k]
        cand = masked[order[:k + 1]]
        cand = cand[np.isfinite(cand)]
        if len(cand) > 1:
            margin[t] = min(margin[t], np.min(cand[:-1] - cand[1:]))
        I[t] = sel
        W[t] = s[t, sel] * scaling
    return (W, I, margin) if with_margin else (W, I)


def align_block(topk_ids, n_experts, block_size):
    """topk_ids [T, k] (or flat) -> (sorted_token_idxes [n_padded], expert_ids [n_padded / block], n_padded,
    cu_sum [E + 1]): experts ascending, an expert's flat indices ascending, padded with n_flat to a multiple of
    block_size; empty experts get no block; ids outside [0, E) are dropped."""
    ids = np.asarray(topk_ids).reshape(-1)
    n_flat = ids.size
    sorted_idx, expert_ids, cu = [], [], [0]
    for e in range(n_experts):
        mine = np.nonzero(ids == e)[0]
        if mine.size:
            nb = -(-mine.size // block_size)
            sorted_idx += list(mine) + [n_flat] * (nb * block_size - mine.size)
            expert_ids += [e] * nb
        cu.append(len(sorted_idx))
    return (np.asarray(sorted_idx, np.int32), np.asarray(expert_ids, np.int32), len(sorted_idx),
            np.asarray(cu, np.int32))


def align_capacity(n_flat, n_experts, block_size):
    """the documented bound: at most min(E, n_flat) experts are non-empty, each pads at most block_size - 1"""
    m = min(n_flat, n_experts)
    blocks = (n_flat + m * (block_size - 1)) // block_size
    return blocks * block_size, blocks


def adversarial_assignments(T, k, n_experts):
    """topk_ids [T, k] that stress the capacity bound: everything to one expert; one entry per expert (round
    robin); the first T * k experts once each."""
    n = T * k
    return {
        "one_expert": np.full((T, k), n_experts - 1, np.int32),
        "round_robin": (np.arange(n, dtype=np.int32) % n_experts).reshape(T, k),
        "spread": (np.arange(n, dtype=np.int32) * max(1, n_experts // max(n, 1)) % n_experts).reshape(T, k),
    }


def moe_sum(x):
    """[T, k, dim] -> [T, dim] float64 (the fp32 order j = 0..k-1 is within an ulp of this)"""
    return np.asarray(x, np.float64).sum(axis=1)
