"""References, input builders and case tables of the exact tie and boundary tests of the vocabulary-row kernels
(csrc/sampling.hip, csrc/rejection.hip, csrc/vocab_row.h): what tests/test_vocab_exact_gpu.py runs on the device and
what tests/test_vocab_exact_cpu.py checks the conditions, the references and the mutants on without one.  Imports no
GPU code.

Input families (include/slm_hip.h sections 8 and 9 are the contract):

  plateau rows   a few LEVELS (values exact in f16, bf16 and f32: small multiples of 1/4) at chosen id sets over a
                 FLOOR of -200 (-400 under temperature 2).  expf(floor - m) is 0 in fp32 (floor' - m <= -110 is
                 asserted per row), so the floor is finite but carries exactly zero mass.  The kept set, the top-n
                 order and the greedy token follow from integers: sort by (level desc, id asc).
  exact params   freq +-0.5, pres 0.5, rep 2, temperature 0.5 / 2 / 0: every penalised or scaled value is exact in
                 all three types, so penalties move tokens between plateaus exactly.
  top-p          either the MIDPOINT of two neighbouring exclusive cumulative masses (margin >= 1e-4, asserted in
                 float64 on the CPU), or an EQUALITY row: the survivors are one plateau of 2^a tokens and top_p is
                 j / 2^a, so every mass is 2^40 units and rank j has mass-before == top_p exactly (kept; j + 1 not).
  sampled rows   the survivors are one plateau: every exp(x - m) is 1 and the token is the survivor with the largest
                 24-bit uniform of its Philox word (stream 0, the row's position), lowest id on equal words.  E =
                 -ln(u) comes from logf / log1pf, which are not correctly rounded, so the table keeps the winner
                 >= 256 units (2^-16 of u) ahead of the runner-up -- orders of magnitude beyond their error.
  rejection      acceptance ratios that are exact (probability form: p_d = r / 2, q_d = 1 / 2; logits form: one
                 plateau of 2^a tokens so p_d = 2^-a, q_d searched so that fl(p_d / q_d) is the wanted float), with
                 the uniform EQUAL to the ratio (must reject) or one fp32 step apart (must accept); recovered tokens
                 where max(p - q, 0) takes one positive value on a chosen set (an integer comparison of stream-2
                 uniforms, same 256-unit margin); greedy ties; masks; strides of every alignment class.

The reference below is written independently of tests/sampling_ref.py and tests/rejection_ref.py (sort-based
selection, float64 masses); only Philox is imported from there (it is pinned to rocRAND on the CPU).  `mut` plants
one mistake in it: the CPU test shows that the tables tell every such mutant from the contract.

MEASURED on an MI355X (gfx950): probs on single-plateau survivors is bit-equal to float32(1) / float32(count) in
every case (0 ulp; PROBS_ULP_BAR below stays 0).
"""
import functools
from collections import namedtuple

import numpy as np

from tests.sampling_ref import philox_words, uniform24

F32 = np.float32
DTYPES = ("f16", "bf16", "f32")
FLOOR = -200.0
ZERO_MASS_BELOW = -110.0   # expf(x) == 0 in fp32 below -103.98 (also with flushed denormals: below -87.4)
RACE_MARGIN = 256          # 24-bit uniform units between the race's winner and its runner-up
TP_MARGIN = 1e-4
PROBS_ULP_BAR = 0          # measured distance of probs from float32(1) / float32(count); see the docstring
LP_ABS, LP_REL = 2e-4, 1e-5    # test_sampling_gpu.py's tolerance for logprobs and multi-level probs

SAMPLING_MUTANTS = ("tie_high", "whole_plateau", "topp_lt", "topp_whole_row", "no_clamp", "no_rank0", "race_all",
                    "race_stream", "race_pos", "topn_nofilter", "negzero_below", "pad_penalised", "count0",
                    "rep_swapped", "temp0")
REJECTION_MUTANTS = ("accept_le", "pos_fixed", "streams_swapped", "recover_p", "greedy_high", "mask_at_f",
                     "oob_accepted")


def exact_in(values, dtype):
    """every value is representable in `dtype` ("f16" | "bf16" | "f32"); -inf counts"""
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)]
    f = v.astype(F32)
    if not np.array_equal(f.astype(np.float64), v):
        return False
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return bool(np.array_equal(f.astype(np.float16).astype(F32), f))
    if dtype == "bf16":
        return not bool((f.view(np.uint32) & 0xFFFF).any())
    return True


# ---------------------------------------------------------------------------------------------------------------------
# sampling: rows, calls, the reference
# ---------------------------------------------------------------------------------------------------------------------
# levels: ((value, ids), ...); pen: ((id, count), ...) the row of the penalty table IN FULL (padding beyond lens
# included); tp_kind: None | "mid" | "eq" (the CPU test checks the margin or the equality condition accordingly);
# cut: the row claims its top-k cut or top-p crossing falls strictly inside a run of equal keys (index select runs)
_ROW_DEFAULTS = dict(levels=(), floor=FLOOR, freq=None, pres=None, rep=None, temp=None, top_k=None, top_p=None,
                     pen=(), lens=0, do_sample=False, seed=0, pos=0, tp_kind=None, cut=False, tag="")
SRow = namedtuple("SRow", list(_ROW_DEFAULTS))
# entry: sample | process (out of place) | inplace (full: temperature or a filter present) | sparse_fp | sparse_rep
#        (the apply_*_penalty forms) | temp (apply_temperature_penalty)
SCase = namedtuple("SCase", "name V entry rows n_top max_unique pad_in pad_out probs dtypes")


def R(**kw):
    d = dict(_ROW_DEFAULTS)
    d.update(kw)
    d["levels"] = tuple((float(v), tuple(int(i) for i in ids)) for v, ids in d["levels"])
    d["pen"] = tuple((int(i), int(c)) for i, c in d["pen"])
    return SRow(**d)


def row_values(V, row):
    x = np.full(V, row.floor, F32)
    for v, ids in row.levels:
        x[list(ids)] = F32(v)
    return x


def call_params(case):
    """The per-call tensors as host arrays (None = not passed): a parameter travels iff some row sets it; the other
    rows get its neutral value."""
    rows = case.rows
    n = len(rows)

    def col(name, neutral, dt):
        if all(getattr(r, name) is None for r in rows):
            return None
        return np.array([neutral if getattr(r, name) is None else getattr(r, name) for r in rows], dtype=dt)
    p = dict(frequency_penalties=col("freq", 0.0, F32), presence_penalties=col("pres", 0.0, F32),
             repetition_penalties=col("rep", 1.0, F32), temperatures=col("temp", 1.0, F32),
             top_k=col("top_k", -1, np.int64), top_p=col("top_p", 1.0, F32))
    if case.max_unique > 0:
        ids = np.zeros((n, case.max_unique), np.int64)
        cnt = np.zeros((n, case.max_unique), np.int32)
        for r, row in enumerate(rows):
            assert len(row.pen) <= case.max_unique, case.name
            for j, (i, c) in enumerate(row.pen):
                ids[r, j], cnt[r, j] = i, c
        p.update(unique_token_ids=ids, unique_token_counts=cnt,
                 unique_token_lens=np.array([r.lens for r in rows], np.int32))
    if case.entry == "sample":
        p.update(do_sample=np.array([r.do_sample for r in rows], bool),
                 seeds=np.array([r.seed for r in rows], np.int64),
                 positions=np.array([r.pos for r in rows], np.int32))
    return p


def _order(key, high=False):
    idx = np.arange(key.size)
    return np.lexsort((-idx if high else idx, -key))


def ref_row(case, r, mut=""):
    """Steps 1-7 of slm_hip.h section 8 for row r of the call, plainly.  Returns vals (fp32 after steps 1-3), keep,
    token, top_ids, top_lp, logprob, probs (float64)."""
    row, P, V = case.rows[r], call_params(case), case.V
    v = row_values(V, row)
    g = lambda name: None if P.get(name) is None else P[name][r]  # noqa: E731
    freq, pres, rep, temp = g("frequency_penalties"), g("presence_penalties"), g("repetition_penalties"), \
        g("temperatures")
    if case.max_unique > 0 and (freq is not None or pres is not None or rep is not None):
        n = min(max(int(row.lens), 0), case.max_unique)
        if mut == "pad_penalised":
            n = case.max_unique
        ids, cnt = P["unique_token_ids"][r], P["unique_token_counts"][r]
        for j in range(n):
            i, c = int(ids[j]), int(cnt[j])
            if not 0 <= i < V:
                continue
            t = v[i]
            if (freq is not None or pres is not None) and (c > 0 or mut == "count0"):
                if freq is not None:
                    t = F32(t - F32(F32(c) * freq))
                if pres is not None:
                    t = F32(t - pres)
            if rep is not None:
                neg = bool(t < 0) != (mut == "rep_swapped")
                t = F32(t * rep) if neg else F32(t / rep)
            v[i] = t
    if temp is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = F32(1) if (temp == 0 and mut != "temp0") else F32(F32(1) / temp)
            v = (v * inv).astype(F32)
    key = v.astype(np.float64) + 0.0
    if mut == "negzero_below":
        key = np.where((v == 0) & np.signbit(v), -2.0 ** -60, key)
    order = _order(key)
    keep = np.ones(V, bool)
    k = g("top_k")
    topk_on = k is not None and 0 < int(k) < V
    if topk_on:
        ok = _order(key, high=True) if mut == "tie_high" else order
        keep[ok[int(k):]] = False
        if mut == "whole_plateau":
            keep[key == key[ok[int(k) - 1]]] = True
    tp = g("top_p")
    if tp is not None and tp < 1:
        tpv = float(tp) if mut == "no_rank0" else max(float(tp), 0.0)   # a negative top_p counts as 0
        surv = order if mut == "topp_whole_row" else order[keep[order]]
        with np.errstate(invalid="ignore"):
            mass = np.exp(key[surv] - key[order[0]])
        excl = np.concatenate([[0.0], np.cumsum(mass / mass.sum())[:-1]])
        kept = excl < tpv if mut == "topp_lt" else excl <= tpv
        if mut != "no_rank0":
            kept[0] = True
        keep2 = np.zeros(V, bool)
        keep2[surv[kept]] = True
        last = int(kept.sum()) - 1
        if mut == "no_clamp" and topk_on and last >= 0 and \
                (last + 1 == surv.size or key[surv[last + 1]] != key[surv[last]]):
            keep2[key == key[surv[last]]] = True   # the crossing is the run's last survivor: the whole run returns
            keep = keep2
        else:
            keep = keep & keep2
    m = key[order[0]]
    with np.errstate(invalid="ignore", divide="ignore"):
        live = keep & (key - m > ZERO_MASS_BELOW)   # the survivors that carry mass (the floor and -inf carry none)
        mass = np.where(live, np.exp(key - m), 0.0)
        s = mass.sum()
        probs = mass / s
        logp = np.where(keep, key - m - np.log(s), -np.inf)
    token = int(order[0])
    if row.do_sample:
        cand = np.nonzero(key == m)[0] if mut == "race_all" else np.nonzero(live)[0]
        u = uniform24(philox_words(row.seed, row.pos + (mut == "race_pos"), cand, stream=int(mut == "race_stream")))
        token = int(cand[np.lexsort((cand, -u))[0]]) if cand.size else token
    tkey = key if mut == "topn_nofilter" else np.where(keep, key, -np.inf)
    top_ids = _order(tkey)[:case.n_top]
    with np.errstate(invalid="ignore"):
        top_lp = np.where(np.isinf(tkey[top_ids]), -np.inf, tkey[top_ids] - m - np.log(s))
    return dict(vals=v, keep=keep, token=token, top_ids=top_ids, top_lp=top_lp, logprob=float(logp[token]), probs=probs,
                live=live, excl_key=key, order=order)


@functools.lru_cache(maxsize=None)
def _ref_cached(name, r):
    return ref_row(S_BY_NAME[name], r)


def expected(case, r):
    """The contract's outputs of row r (cached: shared by the dtypes and never modified by the tests)."""
    return _ref_cached(case.name, r)


def expected_processed(case, r):
    e = expected(case, r)
    return e["vals"] if case.entry.startswith("sparse") else np.where(e["keep"], e["vals"], F32(-np.inf)).astype(F32)


def survivors_one_plateau(case, r):
    e = expected(case, r)
    return np.unique(e["excl_key"][e["live"]]).size == 1


def race_gap(case, r):
    """24-bit units between the two best uniforms among the survivors (0 with one survivor: nothing to race)"""
    row, e = case.rows[r], expected(case, r)
    cand = np.nonzero(e["live"])[0]
    u = np.sort(uniform24(philox_words(row.seed, row.pos, cand)))
    return int(u[-1] - u[-2]) if u.size > 1 else RACE_MARGIN


def topp_margin(case, r):
    """min |mass before rank j - top_p| over the ranks of the top-k survivors, float64"""
    e, P = expected(case, r), call_params(case)
    k, V = P["top_k"][r] if P["top_k"] is not None else -1, case.V
    key, order = e["excl_key"], e["order"]
    surv = order[:int(k)] if 0 < int(k) < V else order
    mass = np.exp(key[surv] - key[order[0]])
    excl = np.concatenate([[0.0], np.cumsum(mass / mass.sum())[:-1]])
    return float(np.abs(excl - float(P["top_p"][r])).min()), surv, mass


def index_passes(V):
    """passes of the index select of vocab_row.h's radix_select when a cut falls strictly inside a run"""
    nb = 1
    while (1 << nb) < V:
        nb += 1
    return (nb - 1) // 8 + 1


def dynamic_lds_bytes(case):
    """the bitmap + prefix table of a full call with penalties (sampling.hip's launch)"""
    pen = case.max_unique > 0 and any(x is not None for r in case.rows for x in (r.freq, r.pres, r.rep))
    return 2 * ((case.V + 31) // 32) * 4 if pen and not case.entry.startswith("sparse") else 0


# ---- id sets --------------------------------------------------------------------------------------------------------
def edge_ids(V, n=16):
    """n ids: the lowest and highest, both sides of the bitmap-word edge 31 / 32, of 255 / 256 and 65535 / 65536"""
    want = [0, 1, 31, 32, 33, V - 1, V - 2, 254, 255, 256, 257, 65534, 65535, 65536, 65537, 63, 64]
    ids = []
    for i in want:
        if 0 <= i < V and i not in ids:
            ids.append(i)
    i = 120
    while len(ids) < n:
        if i % V not in ids:
            ids.append(i % V)
        i += 37
    return tuple(sorted(ids[:n]))


def word_run(V, avoid=(), n=16):
    """n ids inside ONE 32-id bitmap word (word 3; word 0 of a small vocabulary), none of them in `avoid`"""
    w = 3 if V >= 128 else 0
    ids = [i for i in range(32 * w + 2, 32 * w + 31) if i < V and i not in avoid][:n]
    assert len(ids) == n
    return tuple(ids)


def free_ids(V, used, n, start=34):
    ids = [i for i in range(start, V) if i not in used][:n]
    assert len(ids) == n
    return tuple(ids)


def stride_class_ids(V):
    """one id per thread-stride class i mod 1024, spread over the row"""
    per = V // 1024
    return tuple(sorted(c + 1024 * ((c * 7 + 3) % per) for c in range(1024)))


def _seed_with_gap(V, row_fn, pos):
    """the first seed whose race over the row's survivors has the margin (a property of the table, not of a kernel)"""
    for seed in range(1, 200):
        row = row_fn(seed)
        case = SCase("_probe", V, "sample", (row,), 0, 0, 0, 0, False, DTYPES)
        e = ref_row(case, 0)
        cand = np.nonzero(e["live"])[0]
        u = np.sort(uniform24(philox_words(seed, pos, cand)))
        if u.size < 2 or u[-1] - u[-2] >= RACE_MARGIN:
            return row
    raise AssertionError("no seed with the race margin")


def _sampled(V, pos, **kw):
    return _seed_with_gap(V, lambda seed: R(do_sample=True, seed=seed, pos=pos, **kw), pos)


def _mid_tp(V, keep_ranks, **kw):
    """top_p = the midpoint of mass-before of ranks keep_ranks - 1 and keep_ranks: keeps ranks 0 .. keep_ranks - 1"""
    probe = SCase("_probe", V, "sample", (R(top_p=0.5, **kw),), 0, 0, 0, 0, False, DTYPES)
    _, _, mass = topp_margin_raw(probe)
    excl = np.concatenate([[0.0], np.cumsum(mass / mass.sum())[:-1]])
    return float(F32((excl[keep_ranks - 1] + excl[keep_ranks]) / 2))


def topp_margin_raw(case):
    e, P = ref_row(case, 0), call_params(case)
    k = P["top_k"][0] if P["top_k"] is not None else -1
    surv = e["order"][:int(k)] if 0 < int(k) < case.V else e["order"]
    return e, surv, np.exp(e["excl_key"][surv] - e["excl_key"][e["order"][0]])


def filter_rows(V, which=None):
    """The rows of a call without penalties at vocab V >= 63; `which`: a subset of their tags."""
    A = edge_ids(V)                    # top plateau: 16 = 2^4 ids
    B = word_run(V, A)
    lvA = ((1.0, A),)
    lvAB = ((1.0, A), (0.0, B))
    nz = free_ids(V, set(A) | set(B), 4)
    rows = [
        R(tag="k_inside", levels=lvAB, top_k=8, cut=True),
        R(tag="k_end_p_mid", levels=lvAB, top_k=32, top_p=_mid_tp(V, 19, levels=lvAB, top_k=32), tp_kind="mid",
          cut=True),
        R(tag="p_mid_levels", levels=((2.0, A[:3]), (1.0, A[3:]), (0.0, B)), top_k=16,
          top_p=_mid_tp(V, 2, levels=((2.0, A[:3]), (1.0, A[3:]), (0.0, B)), top_k=16), tp_kind="mid", cut=True),
        _sampled(V, 11, tag="p_eq", levels=lvA, top_p=5 / 16, tp_kind="eq", cut=True),
        _sampled(V, 12, tag="both_before", levels=lvA, top_k=8, top_p=3 / 8, tp_kind="eq", cut=True),
        R(tag="both_at", levels=lvA, top_k=8, top_p=7 / 8, tp_kind="eq", cut=True),
        _sampled(V, 13, tag="both_past", levels=lvA, top_k=8, top_p=float(F32(1) - F32(2.0 ** -24)), tp_kind="eq",
                 cut=True),
        R(tag="p_zero", levels=lvAB, top_p=0.0, top_k=V + 1, tp_kind="zero", cut=True),
        R(tag="p_negative", levels=lvAB, top_p=-0.5, tp_kind="zero", cut=True),
        R(tag="p_below_one", levels=lvA, top_p=float(F32(1) - F32(2.0 ** -24)), top_k=0, tp_kind="eq"),
        R(tag="k_in_floor", levels=lvA, top_k=20, cut=True),
        R(tag="k_one", levels=lvAB, top_k=1, cut=True),
        R(tag="k_vm1", levels=lvAB, top_k=V - 1, cut=True),
        R(tag="k_v", levels=lvAB, top_k=V),
        R(tag="k_neg", levels=lvAB, top_k=-1, top_p=1.0),
        _sampled(V, 14, tag="k_end_sampled", levels=lvAB, top_k=16),
        # -0 and +0 share a rank: the lower id wins whatever its sign, and the sign survives into `processed`
        R(tag="neg_zero", levels=((-0.0, nz[:2]), (0.0, nz[2:]), (-1.0, B)), top_k=3, cut=True),
        R(tag="temp_half", levels=lvAB, temp=0.5, top_k=8, cut=True),
        R(tag="temp_two", levels=((4.0, A), (-0.0, B)), floor=2 * FLOOR, temp=2.0, top_k=16 + 4, cut=True),
        R(tag="temp_zero", levels=lvAB, temp=0.0, top_k=16),
    ]
    if V >= 2048:
        C = stride_class_ids(V)        # 2^10 ids, one per thread of the workgroup
        rows += [R(tag="stride_k", levels=((1.0, C),), top_k=512, cut=True),
                 _sampled(V, 15, tag="stride_p_eq", levels=((1.0, C),), top_p=700 / 1024, tp_kind="eq", cut=True)]
    if which is not None:
        rows = [r for r in rows if r.tag in which]
        assert len(rows) == len(which), (V, which)
    return tuple(rows)


def tiny_rows(V):
    """V = 1 and V = 2: every id is on the plateau"""
    ids = tuple(range(V))
    lv = ((0.0, ids),)
    rows = [R(tag="plain", levels=lv), R(tag="k_one", levels=lv, top_k=1, cut=V > 1),
            R(tag="k_v", levels=lv, top_k=V), R(tag="k_vp1", levels=lv, top_k=V + 1),
            R(tag="p_zero", levels=lv, top_p=0.0, tp_kind="zero", cut=V > 1),
            R(tag="p_eq", levels=lv, top_p=0.5, tp_kind="eq"),
            R(tag="p_quarter", levels=lv, top_p=0.25, tp_kind="eq", cut=V > 1),
            R(tag="sampled", levels=lv, do_sample=True, seed=5, pos=9),
            R(tag="sampled_k1", levels=lv, do_sample=True, seed=6, pos=9, top_k=1, cut=V > 1)]
    return tuple(rows)


def neg_inf_rows(V):
    """Rows as LogitsProcessor leaves them (filtered = -inf): what Sampler.forward gets, every filter neutral; and
    the same rows filtered once more (a -inf carries no mass, is never drawn, and ranks last by id)"""
    A = edge_ids(V)
    B = word_run(V, A)
    ninf = -np.inf
    return (R(tag="inf_one_plateau", levels=((1.0, A[:6]),), floor=ninf),
            _sampled(V, 21, tag="inf_sampled", levels=((1.0, A[:8]),), floor=ninf),
            R(tag="inf_two_levels", levels=((1.0, A[:4]), (0.0, B[:4])), floor=ninf),
            R(tag="inf_single", levels=((-3.0, (V - 1,)),), floor=ninf),
            R(tag="inf_k_inside", levels=((1.0, A[:8]),), floor=ninf, top_k=4, cut=True),
            R(tag="inf_k_in_floor", levels=((1.0, A[:4]),), floor=ninf, top_k=6, cut=True),
            _sampled(V, 22, tag="inf_p_eq", levels=((1.0, A[:8]),), floor=ninf, top_p=3 / 8, tp_kind="eq", cut=True))


def pen_rows(V, mu):
    """The rows of a call with penalties: per-row freq / pres / rep, tables of `mu` entries, lens in and out of
    [0, mu].  Values: T = 1.0 (16 edge ids), H = 2.0, N = -0.5, B = 0.0 (a run inside one bitmap word)."""
    T = edge_ids(V)
    B = word_run(V, T)
    HN = free_ids(V, set(T) | set(B), 4)
    H, N = HN[:2], HN[2:]
    used = set(T) | set(B) | set(H) | set(N)
    fl = [i for i in range(70, 70 + 4 * mu + 400) if i % V not in used and i < V][:max(mu, 8)]
    lv = ((1.0, T), (0.0, B), (2.0, H), (-0.5, N))
    lvTB = ((1.0, T), (0.0, B))
    pad = lambda pen: tuple(pen)[:mu] + ((T[1], 7),) * max(0, mu - len(pen))  # noqa: E731  padding names a T token
    if mu == 1:
        one = ((T[2], 1),)
        return (R(tag="mu1_len1", levels=lvTB, freq=0.5, pres=0.5, pen=one, lens=1, top_k=8, cut=True),
                R(tag="mu1_neg", levels=lvTB, freq=0.5, pres=0.5, pen=one, lens=-3, top_k=8, cut=True),
                R(tag="mu1_zero", levels=lvTB, rep=2.0, pen=one, lens=0, top_k=8, cut=True),
                R(tag="mu1_over", levels=lvTB, rep=2.0, pen=one, lens=8, top_k=8, cut=True))
    full = tuple((i, 0) for i in fl[:mu - 4]) + tuple((t, 1) for t in T[4:8])   # mu entries, all within lens
    return (
        # 2.0 - 0.5 - 0.5 lands on T; 1.0 - 1.0 leaves T for B; a count of 0 is not penalised
        R(tag="fp_in_out", levels=lv, freq=0.5, pres=0.5, pen=pad(((H[0], 1), (T[2], 1), (H[1], 0))), lens=3,
          top_k=1 + 8, cut=True),
        # a negative frequency penalty lifts a B token into the top plateau; the race runs over the new plateau
        _sampled(V, 31, tag="fp_lift", levels=lvTB, freq=-0.5, pen=pad(((B[3], 2),)), lens=1, top_k=9, cut=True),
        # rep with counts of 0: positive / 2, negative * 2, +0 / 2; ids on word edges; -1 and V are skipped
        R(tag="rep_edges", levels=lv, freq=0.5, pres=0.5, rep=2.0,
          pen=pad(((0, 0), (31, 0), (32, 0), (V - 1, 0), (H[0], 0), (N[0], 0), (-1, 0), (V, 0), (B[0], 0))), lens=9,
          top_k=1 + 6, cut=True),
        R(tag="len_neg", levels=lv, freq=0.5, pres=0.5, rep=2.0, pen=pad(((0, 1), (31, 1), (H[0], 1))), lens=-3,
          top_k=2 + 8, cut=True),
        R(tag="len_zero", levels=lv, rep=2.0, pen=pad(((0, 1), (H[1], 1))), lens=0, top_k=2 + 8, cut=True),
        R(tag="len_full", levels=lvTB, freq=0.5, pres=0.5, rep=2.0, pen=full, lens=mu, top_k=6, cut=True),
        R(tag="len_over", levels=lvTB, freq=0.5, pres=0.5, rep=2.0, pen=full, lens=mu + 7, top_k=6, cut=True),
    )


def _strip_filters(rows, keep_temp=False):
    return tuple(r._replace(top_k=None, top_p=None, temp=r.temp if keep_temp else None, do_sample=False, cut=False,
                            tp_kind=None) for r in rows)


def _only(rows, keep_fp, keep_rep):
    out = []
    for r in rows:
        if keep_fp and r.freq is None and r.pres is None:
            continue
        if keep_rep and r.rep is None:
            continue
        out.append(r._replace(freq=r.freq if keep_fp else None, pres=r.pres if keep_fp else None,
                              rep=r.rep if keep_rep else None))
    return tuple(out)


def _sampling_cases():
    out = []

    def add(name, V, entry, rows, n_top=0, mu=0, pad_in=0, pad_out=0, probs=False, dtypes=DTYPES):
        out.append(SCase(name, V, entry, tuple(rows), min(n_top, V), mu, pad_in, pad_out, probs, dtypes))
    # ---- no penalties: every vocabulary at which the index select changes its pass count, and the limits ---------
    n_tops = {63: 20, 255: 5, 256: 1, 257: 20, 1023: 63, 1024: 5, 1025: 20, 65536: 5, 65537: 20}
    for V in (1, 2):
        add(f"sample_V{V}", V, "sample", tiny_rows(V), n_top=V, probs=True)
    for V, nt in n_tops.items():
        add(f"sample_V{V}", V, "sample", filter_rows(V), n_top=min(nt, 20), probs=True)
    add("sample_V63_ntopV", 63, "sample", filter_rows(63, ("k_inside", "both_at", "p_zero")), n_top=20)
    add("sample_V20_ntopV", 20, "sample", (R(levels=((1.0, (3, 7, 19)),), top_k=2, cut=True, tag="k_inside"),
                                           R(levels=((1.0, (0, 19)),), top_p=0.0, tp_kind="zero", cut=True, tag="p0")),
        n_top=20, probs=True)
    big = ("k_inside", "both_at", "stride_k", "stride_p_eq")
    add("sample_V2p19", 2 ** 19, "sample", filter_rows(2 ** 19, big), n_top=20, probs=True)
    add("sample_V2p22", 2 ** 22, "sample", filter_rows(2 ** 22, ("k_end_p_mid", "both_past")), n_top=5,
        dtypes=("bf16",))
    # ---- entry points and strides ----------------------------------------------------------------------------------
    sub = ("k_inside", "k_end_p_mid", "both_at", "k_in_floor", "neg_zero", "temp_two", "k_neg")
    add("process_V1025", 1025, "process", filter_rows(1025, sub))
    add("process_V1025_strided", 1025, "process", filter_rows(1025, sub), pad_in=7, pad_out=13)
    add("inplace_V257", 257, "inplace", filter_rows(257, sub))
    add("inplace_V65537_strided", 65537, "inplace", filter_rows(65537, sub), pad_in=9, pad_out=9)
    add("sample_V1025_strided", 1025, "sample", filter_rows(1025, sub), n_top=5, pad_in=5, pad_out=3, probs=True)
    add("temp_V1025", 1025, "temp", _strip_filters(filter_rows(1025, ("temp_half", "temp_two", "temp_zero")), True),
        pad_in=3, pad_out=3)
    # ---- -inf inputs, filters neutral -------------------------------------------------------------------------------
    for V in (257, 65537):
        add(f"neginf_V{V}", V, "sample", neg_inf_rows(V), n_top=20, probs=True)
    # ---- penalties: the bitmap in dynamic LDS up to and beyond 48 KiB ------------------------------------------------
    for V in (255, 1025, 32769, 196608, 196609, 262144, 2 ** 19):
        add(f"pen_V{V}", V, "sample", pen_rows(V, 64), n_top=5, mu=64, probs=V <= 32769)
    add("pen_V1025_mu1", 1025, "sample", pen_rows(1025, 1), n_top=5, mu=1, probs=True)
    add("pen_V32769_mu1500", 32769, "sample", pen_rows(32769, 1500), n_top=20, mu=1500)
    add("pen_process_V196609", 196609, "process", pen_rows(196609, 64), mu=64, pad_out=5)
    add("pen_inplace_V1025_strided", 1025, "inplace", pen_rows(1025, 64), mu=64, pad_in=7, pad_out=7)
    for V, mu in ((255, 64), (32769, 1500), (262144, 64)):
        base = _strip_filters(pen_rows(V, mu))
        add(f"sparse_fp_V{V}", V, "sparse_fp", _only(base, True, False), mu=mu, pad_in=3, pad_out=3)
        add(f"sparse_rep_V{V}", V, "sparse_rep", _only(base, False, True), mu=mu, pad_in=3, pad_out=3)
    return tuple(out)


SAMPLING = _sampling_cases()
S_BY_NAME = {c.name: c for c in SAMPLING}
assert len(S_BY_NAME) == len(SAMPLING)


# ---------------------------------------------------------------------------------------------------------------------
# rejection
# ---------------------------------------------------------------------------------------------------------------------
# align: the byte alignment class of every target / draft row: 16 | 8 | 0 (unaligned); interleaved: the target is a
# [k + 1, n, V] buffer viewed as [n, k + 1, V]; seqs: per sequence a dict (see _seq)
RCase = namedtuple("RCase", "name V k form mask lp n_top philox t_align d_align interleaved seqs dtypes")
PAD_VALUE = 1.0e4     # what the padding between strided rows holds: larger than any level, so a read of it shows


def step_up(x):
    return F32(np.nextafter(F32(x), F32(np.inf)))


def step_down(x):
    return F32(np.nextafter(F32(x), F32(-np.inf)))


def accept_uniform(seed, pos, j):
    """u = ((x >> 8) + 0.5) 2^-24 rounded to fp32, x = word 0 of stream 1 at position pos + j"""
    m = int(uniform24(philox_words(seed, (pos + j) & 0xFFFFFFFF, [0], stream=1))[0])
    return F32(F32(F32(m) + F32(0.5)) * F32(2.0 ** -24))


def q_for_ratio(p, ratio):
    """a float q with fl(p / q) == ratio exactly, or None"""
    q0 = F32(F32(p) / F32(ratio))
    q = q0
    for _ in range(6):
        q = step_down(q)
    for _ in range(13):
        if F32(F32(p) / q) == F32(ratio):
            return q
        q = step_up(q)
    return None


def _seq(V, k, f, form, philox, seed, pos, a, greedy=False, oob_at=None, plateau=None, recover=None):
    """One sequence whose first rejected row is f (k: none).  Rows after f alternate accept / reject (they show in
    the unmasked and logprob forms).  Every sampled row sits ON the acceptance boundary: a rejecting row has
    u == ratio, an accepting one is one fp32 step on the other side."""
    n_pl = 1 << a
    plateau = tuple(plateau if plateau is not None else edge_ids(V, n_pl))
    recover = tuple(recover if recover is not None else plateau[1::2])
    rest = [i for i in plateau if i not in recover]
    accept = [True if j < f else False if j == f else bool((j - f) % 2 == 0) for j in range(k)]
    drafts, rows_t, rows_q, uni = [], [], [], []
    for j in range(k):
        d = rest[j % len(rest)]
        if greedy:                             # a run of equal maxima: the lowest id is the token
            ids = plateau[j % 3:]
            t = np.full(V, FLOOR, F32)
            t[list(ids)] = F32(1.0)
            drafts.append(min(ids) if accept[j] else max(ids))
            rows_t.append(t)
            rows_q.append(np.zeros(V, F32))
            uni.append(F32(0.5))
            continue
        oob = oob_at is not None and j == oob_at[0]
        if oob:
            accept[j] = False
        if philox:
            u = accept_uniform(seed, pos, j)
            ratio = step_up(u) if accept[j] else u
        else:
            ratio = F32(2.0 ** -(1 + j % 3))
            u = step_down(ratio) if accept[j] else ratio
        if form == "probs":
            t = np.zeros(V, F32)
            q = np.zeros(V, F32)
            t[list(plateau)] = F32(0.25)       # p < q off the recovery set
            q[list(plateau)] = F32(0.5)
            t[list(recover)] = F32(0.75)       # p - q = 0.25 on it
            t[d], q[d] = F32(ratio * F32(0.5)), F32(0.5)   # exact: a power-of-two scaling
        else:
            t = np.full(V, FLOOR, F32)
            t[list(plateau)] = F32(0.0)        # p = 2^-a on the plateau, exactly 0 off it
            q = np.zeros(V, F32)
            q[list(plateau)] = F32(1.0)
            q[list(recover)] = F32(0.0)        # p - q = 2^-a on the recovery set
            qd = q_for_ratio(F32(2.0 ** -a), ratio)
            if qd is None or not qd > F32(2.0 ** -a):
                return None                    # this seed's uniform cannot be met exactly: the caller tries the next
            q[d] = qd
        drafts.append((V + 5 if oob_at[1] else -1) if oob else d)
        rows_t.append(t)
        rows_q.append(q)
        uni.append(u)
    if form == "logits":                       # row k: the bonus row (read with logprobs only)
        t = np.full(V, FLOOR, F32)
        t[list(plateau[:2])] = F32(1.0)
        rows_t.append(t)
    return dict(drafts=np.array(drafts, np.int64), target=np.stack(rows_t), draft=np.stack(rows_q),
                uniform=np.array(uni, F32), do_sample=not greedy, seed=seed, pos=pos, bonus=int(plateau[1 % n_pl]),
                accept=accept, f=f, plateau=plateau, recover=recover, a=a)


def _recover_gap(seq, j, V, stream=2):
    u = np.sort(uniform24(philox_words(seq["seed"], (seq["pos"] + j) & 0xFFFFFFFF, np.array(seq["recover"]),
                                       stream=stream)))
    return int(u[-1] - u[-2]) if u.size > 1 else RACE_MARGIN


def _make_seq(V, k, f, form, philox, pos, a, **kw):
    for seed in range(1, 4000):
        s = _seq(V, k, f, form, philox, seed, pos, a, **kw)
        if s is None:
            continue
        if s["do_sample"] and any(_recover_gap(s, j, V) < RACE_MARGIN for j in range(k)):
            continue
        return s
    raise AssertionError(("no seed", V, k, f, form, philox))


def _first_rejections(k):
    return sorted({0, k // 2, k - 1, k})


def _rejection_cases():
    out = []

    def add(name, V, k, form, mask, lp, philox, t_align=16, d_align=16, interleaved=False, n_top=0, a=3, extra=(),
            dtypes=None):
        seqs = [_make_seq(V, k, f, form, philox, 100 + 17 * f, a) for f in _first_rejections(k)]
        seqs += list(extra)
        dt = ("f32",) if form == "probs" else (dtypes or DTYPES)
        out.append(RCase(name, V, k, form, mask, lp, min(n_top, V) if lp else 0, philox, t_align, d_align,
                         interleaved, tuple(seqs), dt))
    V0 = 8203     # odd, > 8 * 1024: a tail group, ids on the thread-stride boundary of every group width
    stride_pl = (0, 4096, 8192, 8195, 8200, 8201, 8202, 4095)        # 2^3 ids: group starts, the tail group, V - 1
    for mask in (False, True):
        for lp in (False, True):
            tag = f"{'masked' if mask else 'unmasked'}_{'lp' if lp else 'nolp'}"
            for k in (1, 4, 16):
                extra = []
                if k == 4:
                    extra = [_make_seq(V0, k, 2, "logits", False, 55, 3, oob_at=(2, True), plateau=stride_pl),
                             _make_seq(V0, k, 0, "logits", False, 56, 3, oob_at=(0, False), plateau=stride_pl),
                             _make_seq(V0, k, 1, "logits", False, 57, 3, greedy=True, plateau=stride_pl)]
                add(f"logits_uniform_k{k}_{tag}", V0, k, "logits", mask, lp, False, n_top=5, extra=extra)
            for k in (1, 4):
                add(f"logits_philox_k{k}_{tag}", 1027, k, "logits", mask, lp, True, n_top=20, a=2)
            if not lp:
                for k in (1, 4, 16):
                    add(f"probs_uniform_k{k}_{tag}", V0, k, "probs", mask, False, False)
                    add(f"probs_philox_k{k}_{tag}", 1027, k, "probs", mask, False, True)
    # ---- alignment classes of the target and the draft rows, independently; interleaved views ------------------------
    for ta in (16, 8, 0):
        for da in (16, 8, 0):
            if (ta, da) == (16, 16):
                continue
            add(f"logits_align_t{ta}_d{da}", V0, 4, "logits", True, False, False, t_align=ta, d_align=da)
            add(f"probs_align_t{ta}_d{da}", V0, 4, "probs", False, False, False, t_align=ta, d_align=da)
    add("logits_interleaved_V8200", 8200, 4, "logits", True, True, False, interleaved=True, n_top=5)
    add("logits_interleaved_V8203", V0, 4, "logits", False, False, False, interleaved=True)
    add("logits_V5", 5, 4, "logits", True, True, False, n_top=5, a=1)
    return tuple(out)


def greedy_rows(V):
    """target rows of all-greedy calls: (row, expected argmax).  Ties go to the lowest id; all -inf gives 0."""
    def mk(ids, floor=FLOOR, val=1.0):
        t = np.full(V, floor, F32)
        t[list(ids)] = F32(val)
        return t
    sets = [(0, V - 1), (V - 1,), (V - 2, V - 1)] + [(i, i + 1, V - 1) for i in (4095, 4096, 4097, 8191, 8192, 8193)]
    rows = [(mk(ids), min(ids)) for ids in sets if min(ids) >= 0 and max(ids) < V and len(set(ids)) == len(ids)]
    rows += [(np.full(V, -np.inf, F32), 0), (mk((V - 1,), floor=-np.inf, val=-3.0), V - 1)]
    if V > 5:
        rows.append((mk((3, 5), val=0.0, floor=-0.0), 0))      # -0 == +0: the lowest id of the whole row
    return rows


REJECTION = _rejection_cases()
R_BY_NAME = {c.name: c for c in REJECTION}
assert len(R_BY_NAME) == len(REJECTION)
GREEDY_V = (1, 5, 1027, 8200, 8203)


def rejection_layout(case, dtype):
    """element offsets and strides of the target and draft buffers: (t_off, t_row, t_seq, d_off, d_row, d_seq)"""
    eb = 4 if dtype == "f32" else 2
    def cls(align, ebytes):   # noqa: E306
        per16 = 16 // ebytes
        return 0 if align == 16 else per16 // 2 if align == 8 else 1
    rows_t = case.k + (1 if case.form == "logits" else 0)
    t_row = (case.V + 7) // 8 * 8 + 8
    d_row = (case.V + 3) // 4 * 4 + 4
    return (cls(case.t_align, eb), t_row, rows_t * t_row + 8, cls(case.d_align, 4), d_row, case.k * d_row + 4)


def ref_rejection(case, s, mut=""):
    """slm_hip.h section 9 for sequence s, plainly.  Returns tokens (unmasked), out (as the call writes them),
    accepted_len, logprobs / top ids / top logprobs (float64; logits form)."""
    q, V, k = case.seqs[s], case.V, case.k
    tgt = q["target"].astype(np.float64)
    tokens = np.zeros(k + 1, np.int64)
    acc = np.zeros(k, bool)
    for j in range(k):
        d = int(q["drafts"][j])
        row = tgt[j] + 0.0
        if case.form == "logits":
            with np.errstate(invalid="ignore"):
                e = np.exp(row - row.max())
            p32 = (e / e.sum()).astype(F32)     # exact here: a plateau of 2^a ones
        else:
            p32 = q["target"][j]
        if not q["do_sample"]:
            best = np.nonzero(row == row.max())[0]
            t = int(best[-1] if mut == "greedy_high" else best[0])
            acc[j] = t == d
            tokens[j] = t
            continue
        pos = q["pos"] + (0 if mut == "pos_fixed" else j)
        s_acc, s_race = (2, 1) if mut == "streams_swapped" else (1, 2)
        if 0 <= d < V:
            if case.philox:
                m = int(uniform24(philox_words(q["seed"], pos & 0xFFFFFFFF, [0], stream=s_acc))[0])
                u = F32(F32(F32(m) + F32(0.5)) * F32(2.0 ** -24))
            else:
                u = q["uniform"][j]
            ratio = F32(p32[d] / q["draft"][j][d])
            acc[j] = bool(u <= ratio) if mut == "accept_le" else bool(u < ratio)
        elif mut == "oob_accepted":
            acc[j] = True
        if acc[j]:
            tokens[j] = d
        else:
            dd = p32.astype(np.float64) if mut == "recover_p" else \
                np.maximum(p32.astype(np.float64) - q["draft"][j].astype(np.float64), 0.0)
            cand = np.nonzero(dd == dd.max())[0] if dd.max() > 0 else np.array([0])
            u24 = uniform24(philox_words(q["seed"], pos & 0xFFFFFFFF, cand, stream=s_race))
            tokens[j] = int(cand[np.lexsort((cand, -u24))[0]])
    tokens[k] = q["bonus"]
    rej = np.nonzero(~acc)[0]
    f = int(rej[0]) if rej.size else k
    out = tokens.copy()
    if case.mask:
        out[(f if mut == "mask_at_f" else f + 1):] = -1
    res = dict(tokens=tokens, out=out, accepted_len=f + 1, accepted=acc)
    if case.form == "logits":
        lps, tids, tlps = [], [], []
        for j in range(k + 1):
            row = tgt[j] + 0.0
            lp = row - row.max() - np.log(np.exp(row - row.max()).sum())
            t = int(tokens[j])
            lps.append(lp[t] if 0 <= t < V else np.nan)
            o = np.lexsort((np.arange(V), -row))[:case.n_top]
            tids.append(o)
            tlps.append(lp[o])
        res.update(logprobs=np.array(lps), top_ids=np.array(tids), top_lp=np.array(tlps))
    return res


def case_counts():
    """cases per path, for the record"""
    from collections import Counter
    c = Counter(x.entry for x in SAMPLING)
    c.update(f"rejection_{x.form}" for x in REJECTION)
    return dict(c)
