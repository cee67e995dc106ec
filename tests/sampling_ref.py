"""numpy restatement of the sampling contract (include/slm_hip.h section 8) -- the oracle of
tests/test_sampling_*.py.  Citations are to the reference tree:

  step 1  frequency / presence   src/kernels/sampling/penalty_kernels.cu:113-143 (the GPU kernel: only
                                 the first lens[r] entries with count > 0; the CPU detail:: version,
                                 logits_processor.h:38-54, also penalises the padding id 0)
  step 2  repetition             penalty_kernels.cu:57-80
  step 3  temperature            penalty_kernels.cu:9-31 (fp32 reciprocal, t == 0 -> 1),
                                 logits_processor.h:190-216
  step 4  top-k                  logits_processor.h:226-262
  step 5  top-p                  logits_processor.h:264-276
  step 6  sample                 src/sampling/sampler.cpp:19-70 (softmax, exponential race, argmax)
  step 7  logprobs / top-n       sampler.cpp:43-56

Every ordering is stable by index (np.lexsort / np.argmax take the first), steps 1-3 are float32
operations one at a time (numpy never contracts), top-p masses are exact (float64 over the float32
exponentials).  Philox4x32-10 is Salmon et al. (SC'11) with the constants of Random123 / rocRAND.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(key: int, ctr):
    """One Philox4x32-10 block: key = 64-bit seed (lo, hi words), ctr = 4 uint32 words (arrays ok)."""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in ctr]
    k0, k1 = np.uint64(key & MASK32), np.uint64((key >> 32) & MASK32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & np.uint64(MASK32), p1 & np.uint64(MASK32),
             ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & np.uint64(MASK32), p0 & np.uint64(MASK32)]
        k0 = (k0 + np.uint64(W0)) & np.uint64(MASK32)
        k1 = (k1 + np.uint64(W1)) & np.uint64(MASK32)
    return c


def philox_words(seed: int, position: int, ids, stream: int = 0) -> np.ndarray:
    """The 32-bit draw of token i: counter (lo32(i >> 2), hi32(i >> 2), position, stream), word i & 3
    == rocRAND philox4x32_10_engine(seed, position | stream << 32, i).next()."""
    i = np.asarray(ids, dtype=np.uint64)
    q = i >> np.uint64(2)
    n = q.shape
    c = philox4x32_10(seed & ((1 << 64) - 1),
                      [q & np.uint64(MASK32), q >> np.uint64(32), np.full(n, position & MASK32, np.uint64),
                       np.full(n, stream & MASK32, np.uint64)])
    w = (i & np.uint64(3)).astype(np.int64)
    out = np.choose(w, c)
    return out.astype(np.uint32)


def uniform24(words) -> np.ndarray:
    """(x >> 8): the 24-bit integer of u = ((x >> 8) + 0.5) 2^-24."""
    return (np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(np.int64)


def exp_draws(words) -> np.ndarray:
    """E = -ln(u) as the kernel evaluates it: -log(u) below 1/2, -log1p(-(1 - u)) above (u and 1 - u are
    exact in float32)."""
    m = uniform24(words)
    lo = m < (1 << 23)
    u = ((m.astype(F32) + F32(0.5)) * F32(2.0 ** -24)).astype(F32)
    v = ((((1 << 24) - 1 - m).astype(F32) + F32(0.5)) * F32(2.0 ** -24)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_lo = -np.log(u)
        e_hi = -np.log1p(-v)
    return np.where(lo, e_lo, e_hi).astype(F32)


def _order(x: np.ndarray) -> np.ndarray:
    """indices by value descending, index ascending (-0 == +0)."""
    return np.lexsort((np.arange(x.size), -(x.astype(np.float64) + 0.0)))


def process_row(x, *, freq=None, pres=None, rep=None, temp=None, top_k=None, top_p=None, ids=None,
                counts=None, n_ids=0):
    """Steps 1-5 for one row: float32 logits in, processed float32 logits (filtered = -inf) out.
    Also returns the exclusive top-p cumsum at each rank (float64) for the boundary allowance."""
    x = np.array(x, dtype=F32)
    V = x.size
    if ids is not None:
        for j in range(n_ids):
            tid = int(ids[j])
            if not 0 <= tid < V:
                continue
            v = x[tid]
            if counts is not None and int(counts[j]) > 0:
                if freq is not None:
                    v = F32(v - F32(F32(int(counts[j])) * F32(freq)))
                if pres is not None:
                    v = F32(v - F32(pres))
            if rep is not None:
                v = F32(v * F32(rep)) if v < 0 else F32(v / F32(rep))
            x[tid] = v
    if temp is not None:
        inv = F32(1.0) if F32(temp) == 0 else F32(F32(1.0) / F32(temp))
        x = (x * inv).astype(F32)
    keep = np.ones(V, bool)
    order = _order(x)
    excl = None
    if top_k is not None and 0 < int(top_k) < V:
        keep[order[int(top_k):]] = False
    if top_p is not None and F32(top_p) < 1:
        m = x[order[0]]
        e = np.where(keep, np.exp((x - m).astype(F32)).astype(F32), F32(0)).astype(np.float64)
        p = e[order] / e.sum()
        excl = np.concatenate([[0.0], np.cumsum(p)[:-1]])
        drop = excl > float(F32(top_p))
        drop[0] = False  # rank 0 is always kept (top_p <= 0 included)
        keep[order[drop]] = False
        excl_at = np.empty(V)
        excl_at[order] = excl
        excl = excl_at
    out = np.where(keep, x, F32(-np.inf)).astype(F32)
    return out, excl


def race_scores(processed, seed: int, position: int):
    """exp(x - max) / E over the survivors (0 elsewhere), float32 -- argmax(probs / E) up to the common
    factor 1 / sum."""
    x = np.asarray(processed, dtype=F32)
    m = x.max()
    e = np.exp((x - m).astype(F32)).astype(F32)
    E = exp_draws(philox_words(seed, position, np.arange(x.size)))
    s = np.where(np.isfinite(x), (e / E).astype(F32), F32(0))
    return s


def sample_row(processed, do_sample: bool, seed: int, position: int) -> int:
    x = np.asarray(processed, dtype=F32)
    if not do_sample:
        return int(np.argmax(x))
    return int(np.argmax(race_scores(x, seed, position)))


def logprobs_row(processed, token: int, n_top: int):
    x = np.asarray(processed, dtype=np.float64)
    m = x.max()
    lse = np.log(np.exp(x - m).sum())
    lp = x - m - lse
    order = _order(np.asarray(processed, dtype=F32))[:n_top]
    return lp[token], lp[order], order
