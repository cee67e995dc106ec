"""numpy restatement of the rejection-sampling contract (include/slm_hip.h section 9) -- the oracle of
tests/test_rejection_*.py.  Citations are to the reference tree:

  acceptance       src/speculative/rejection_sampler.cpp:151-157 (u < p_d / q_d)
  recovered token  rejection_sampler.cpp:159-170 (clamp(p - q, 0), renormalised -- a common factor
                   dropped here -- then Sampler::random_sample: argmax(probs / Exp(1)))
  greedy           rejection_sampler.cpp:192-224 (argmax of the target row, accepted iff equal)
  mask             rejection_sampler.cpp:118-141 (build_accepted_mask)
  logprobs         rejection_sampler.cpp:98-116 (log_softmax of every target row at the unmasked token)

Random numbers: sampling_ref.philox_words with stream 1 (acceptance, word 0) and stream 2 (race, word i),
counter position = positions[s] + j.  Arithmetic is float32 one operation at a time, as the kernel's.
"""
from __future__ import annotations

import numpy as np

from tests import sampling_ref as sref

F32 = np.float32


def target_probs(logits) -> np.ndarray:
    """p_i = expf(l_i - m) / S in float32 (S summed in float32; the kernel's order differs by a few ulp)."""
    x = np.asarray(logits, dtype=F32)
    m = x.max()
    e = np.exp((x - m).astype(F32)).astype(F32)
    s = F32(e.sum(dtype=F32))
    return (e / s).astype(F32)


def acceptance_uniform(seed: int, position: int, j: int) -> F32:
    """u = ((x >> 8) + 0.5) 2^-24, x = word 0 of stream 1 at position + j."""
    x = sref.philox_words(seed, (position + j) & 0xFFFFFFFF, [0], stream=1)
    return F32((sref.uniform24(x)[0] + 0.5) * 2.0 ** -24)


def race_scores(p, q, seed: int, position: int, j: int) -> np.ndarray:
    """max(p_i - q_i, 0) / E_i, float32, E_i from stream 2 at position + j."""
    p, q = np.asarray(p, dtype=F32), np.asarray(q, dtype=F32)
    dd = np.maximum((p - q).astype(F32), F32(0))
    E = sref.exp_draws(sref.philox_words(seed, (position + j) & 0xFFFFFFFF, np.arange(p.size), stream=2))
    return (dd / E).astype(F32)


def validate_seq(draft_ids, draft_probs, target, bonus: int, *, do_sample: bool, seed: int = 0, position: int = 0,
                 uniform=None, target_is_probs: bool = False) -> dict:
    """One sequence: draft_ids [k], draft_probs [k, V] (or None when greedy), target [k + 1, V] logits or
    [k, V] probabilities.  Returns tokens [k + 1] (unmasked), accepted [k], f, accepted_len, and per row
    the acceptance ratio / uniform and the race scores (sampled rejected rows) for tolerance checks."""
    k = len(draft_ids)
    tgt = np.asarray(target, dtype=F32)
    V = tgt.shape[1]
    tokens = np.zeros(k + 1, np.int64)
    accepted = np.zeros(k, bool)
    ratios, us, scores = [None] * k, [None] * k, [None] * k
    for j in range(k):
        d = int(draft_ids[j])
        if not do_sample:
            t = int(np.argmax(tgt[j]))
            accepted[j] = t == d
            tokens[j] = t
            continue
        p = tgt[j] if target_is_probs else target_probs(tgt[j])
        q = np.asarray(draft_probs[j], dtype=F32)
        u = F32(uniform[j]) if uniform is not None else acceptance_uniform(seed, position, j)
        if 0 <= d < V:
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = F32(p[d] / q[d])
            accepted[j] = bool(u < ratio)
            ratios[j], us[j] = ratio, u
        if accepted[j]:
            tokens[j] = d
        else:
            s = race_scores(p, q, seed, position, j)
            scores[j] = s
            tokens[j] = int(np.argmax(s))
    tokens[k] = int(bonus)
    rej = np.nonzero(~accepted)[0]
    f = int(rej[0]) if rej.size else k
    masked = tokens.copy()
    masked[f + 1:] = -1
    return dict(tokens=tokens, masked=masked, accepted=accepted, f=f, accepted_len=f + 1, ratios=ratios, us=us,
                scores=scores)


def build_accepted_mask(accepted) -> np.ndarray:
    """[n, k] -> [n, k + 1]: True up to and including the first rejected row."""
    a = np.asarray(accepted, bool)
    n, k = a.shape
    out = np.zeros((n, k + 1), bool)
    for s in range(n):
        rej = np.nonzero(~a[s])[0]
        f = int(rej[0]) if rej.size else k
        out[s, :f + 1] = True
    return out


def logprobs_rows(target, tokens, n_top: int):
    """log_softmax of each target row (float64 over the float32 values) at tokens[j], and its top-n."""
    x = np.asarray(target, dtype=np.float64)
    lps, tops, ids = [], [], []
    for j in range(x.shape[0]):
        m = x[j].max()
        lp = x[j] - m - np.log(np.exp(x[j] - m).sum())
        t = int(tokens[j])
        lps.append(lp[t] if 0 <= t < x.shape[1] else np.nan)
        order = sref._order(np.asarray(target[j], dtype=F32))[:n_top]
        tops.append(lp[order])
        ids.append(order)
    return np.array(lps), np.array(tops), np.array(ids)
