"""The exact vocabulary-row tests without a GPU: every case of tests/vocab_exact_cases.py meets the conditions its
exactness rests on (levels exact in the dtype, a floor without mass, the top-p margin or the equality condition, the
race margin, acceptance uniforms ON the boundary), reaches the kernel path it names, and gets the same answer from
the plain reference there and from tests/sampling_ref.py / tests/rejection_ref.py.  Then: a reference with one
mistake planted (vocab_exact_cases' `mut`) differs from the contract on at least one case -- the tables would catch
a kernel that made it."""
import numpy as np
import pytest

from tests import rejection_ref as rref
from tests import sampling_ref as sref
from tests import vocab_exact_cases as X

F32 = np.float32
S_CASES = [pytest.param(c, id=c.name) for c in X.SAMPLING]
R_CASES = [pytest.param(c, id=c.name) for c in X.REJECTION]
MUTANT_MAX_V = 1025      # the mutants are shown on the small tables (the large ones repeat their rows)


def _bits(a):
    return np.asarray(a, dtype=F32).view(np.uint32)


def _sparse_by_the_kernels_rule(case, P):
    """sampling.hip's sparse_call: in place, penalties alone"""
    in_place = case.entry in ("inplace", "temp", "sparse_fp", "sparse_rep") and case.pad_in == case.pad_out
    return in_place and all(P[k] is None for k in ("temperatures", "top_k", "top_p"))


def _cut_inside_a_run(e):
    key, keep = e["excl_key"], e["keep"]
    dropped = set(np.unique(key[~keep]).tolist())
    return any(k in dropped for k in np.unique(key[keep]).tolist())


# ---- sampling: conditions, paths, both references -------------------------------------------------------------------
@pytest.mark.parametrize("case", S_CASES)
def test_sampling_case_conditions_paths_and_references(case):
    P = X.call_params(case)
    assert _sparse_by_the_kernels_rule(case, P) == case.entry.startswith("sparse"), case.name
    if case.entry in ("inplace", "temp"):
        assert case.pad_in == case.pad_out
    lds = X.dynamic_lds_bytes(case)
    assert (lds > 0) == (case.max_unique > 0 and not case.entry.startswith("sparse")) and lds <= 128 * 1024
    for r, row in enumerate(case.rows):
        where = (case.name, r, row.tag)
        e = X.expected(case, r)
        x = X.row_values(case.V, row)
        for dt in case.dtypes:   # inputs and every penalised / scaled value: what the kernel reads and writes is exact
            assert X.exact_in(x, dt) and X.exact_in(e["vals"], dt), (where, dt)
        key, m = e["excl_key"], e["excl_key"][e["order"][0]]
        finite = key[np.isfinite(key)]
        assert np.all((finite - m >= -8) | (finite - m <= X.ZERO_MASS_BELOW)), where     # a level, or no mass at all
        assert np.exp(F32(X.ZERO_MASS_BELOW + 6)) == 0 and np.exp(F32(-200)) == 0
        # ---- top-p: margin, equality, or zero ------------------------------------------------------------------
        tp = None if P["top_p"] is None else P["top_p"][r]
        if tp is not None and tp < 1:
            margin, surv, mass = X.topp_margin(case, r)
            if row.tp_kind == "mid":
                assert margin >= X.TP_MARGIN, (where, margin)
            elif row.tp_kind == "eq":    # one plateau of 2^a tokens carries the mass: 2^40 units each, t is exact
                cnt = int((mass > np.exp(X.ZERO_MASS_BELOW)).sum())
                assert cnt & (cnt - 1) == 0 and np.all(mass[:cnt] == 1.0), where
                t = float(tp) * cnt * 2.0 ** 40
                assert t == int(t), where
                kept = int(e["live"].sum())
                assert kept == min(int(float(tp) * cnt) + 1, cnt), (where, kept)     # rank j == top_p * cnt is kept
            else:
                assert row.tp_kind == "zero" and tp <= 0 and int(e["keep"].sum()) == 1, where
        else:
            assert row.tp_kind is None, where
        # ---- the race -----------------------------------------------------------------------------------------------
        if row.do_sample:
            assert X.survivors_one_plateau(case, r) and X.race_gap(case, r) >= X.RACE_MARGIN, where
        # ---- the path: a cut strictly inside a run of equal keys runs the index select -------------------------------
        assert _cut_inside_a_run(e) == row.cut, where
        # ---- the other reference ------------------------------------------------------------------------------------
        g = lambda k: None if P.get(k) is None else P[k][r]  # noqa: E731
        n_ids = min(max(int(row.lens), 0), case.max_unique)
        with np.errstate(invalid="ignore", divide="ignore"):
            out, _ = sref.process_row(x, freq=g("frequency_penalties"), pres=g("presence_penalties"),
                                      rep=g("repetition_penalties"), temp=g("temperatures"), top_k=g("top_k"),
                                      top_p=g("top_p"), ids=g("unique_token_ids"), counts=g("unique_token_counts"),
                                      n_ids=n_ids)
        assert np.array_equal(_bits(out), _bits(X.expected_processed(case, r))), where
        if case.entry == "sample":
            with np.errstate(invalid="ignore", divide="ignore"):
                assert sref.sample_row(out, row.do_sample, row.seed, row.pos) == e["token"], where
                lp, top_v, top_i = sref.logprobs_row(out, e["token"], case.n_top)
            assert lp == pytest.approx(e["logprob"], abs=1e-9), where
            assert np.array_equal(top_i, e["top_ids"]), where
            assert np.array_equal(np.isinf(top_v), np.isinf(e["top_lp"])), where
            fin = np.isfinite(top_v)
            np.testing.assert_allclose(top_v[fin], e["top_lp"][fin], atol=1e-9)


def test_sampling_axes_are_covered():
    """the table reaches what the issue lists: vocabularies, pass counts, both sides of 48 KiB, the penalty table"""
    def vs(pred):
        return {c.V for c in X.SAMPLING if pred(c)}
    assert vs(lambda c: c.max_unique == 0) >= {1, 2, 63, 255, 256, 257, 1023, 1024, 1025, 65536, 65537, 2 ** 19,
                                               2 ** 22}
    full_pen = vs(lambda c: X.dynamic_lds_bytes(c) > 0)
    assert full_pen >= {255, 1025, 32769, 196608, 196609, 262144, 2 ** 19}
    lds = {c.V: X.dynamic_lds_bytes(c) for c in X.SAMPLING if X.dynamic_lds_bytes(c)}
    assert lds[196608] == 48 * 1024 and lds[196609] > 48 * 1024 and lds[2 ** 19] == 128 * 1024
    passes = {X.index_passes(c.V) for c in X.SAMPLING if any(r.cut for r in c.rows)}
    assert passes == {1, 2, 3}
    assert [X.index_passes(v) for v in (2, 256, 257, 65536, 65537, 2 ** 22)] == [1, 1, 2, 2, 3, 3]
    assert {c.entry for c in X.SAMPLING} == {"sample", "process", "inplace", "temp", "sparse_fp", "sparse_rep"}
    assert {c.max_unique for c in X.SAMPLING} >= {1, 64, 1500}
    n_tops = {c.n_top for c in X.SAMPLING}
    assert n_tops >= {1, 5, 20} and any(c.n_top == c.V for c in X.SAMPLING)
    for mu in (1, 64, 1500):
        lens = {r.lens for c in X.SAMPLING if c.max_unique == mu for r in c.rows}
        assert lens >= {-3, 0, mu, mu + 7}, (mu, lens)
    pen_ids = {i for c in X.SAMPLING if c.max_unique == 64 for r in c.rows for i, _ in r.pen[:max(r.lens, 0)]}
    assert pen_ids >= {0, 31, 32, -1} and any(c.V in pen_ids and c.V - 1 in pen_ids for c in X.SAMPLING)
    top_ks = {(r.top_k, c.V) for c in X.SAMPLING for r in c.rows if r.top_k is not None}
    for V in (1025, 65537):
        assert {k for k, v in top_ks if v == V} >= {-1, 1, 8, 16, 20, V - 1, V}
    assert any(k == v + 1 for k, v in top_ks) and any(k == 0 for k, _ in top_ks)
    assert any(c.pad_in and c.pad_out for c in X.SAMPLING if c.entry == "sample")
    assert all(set(c.dtypes) == set(X.DTYPES) for c in X.SAMPLING if c.V < 2 ** 22)
    # more n_top than survivors: the -inf tail is ordered by id
    assert any(c.n_top > int(X.expected(c, r)["keep"].sum()) for c in X.SAMPLING for r in range(len(c.rows))
               if c.entry == "sample" and c.V <= 1025)


def _sampling_outputs(case, r, mut):
    with np.errstate(all="ignore"):
        e = X.ref_row(case, r, mut)
    proc = e["vals"] if case.entry.startswith("sparse") else np.where(e["keep"], e["vals"], F32(-np.inf))
    return _bits(proc).tobytes(), (e["token"] if case.entry == "sample" else 0), \
        (tuple(e["top_ids"].tolist()) if case.entry == "sample" else ())


@pytest.mark.parametrize("mut", X.SAMPLING_MUTANTS)
def test_every_sampling_mutant_fails_a_case(mut):
    caught = [(c.name, row.tag) for c in X.SAMPLING if c.V <= MUTANT_MAX_V for r, row in enumerate(c.rows)
              if _sampling_outputs(c, r, mut) != _sampling_outputs(c, r, "")]
    assert caught, mut
    print(mut, "caught by", len(caught), "rows, e.g.", caught[:3])


# ---- rejection -------------------------------------------------------------------------------------------------------
def _alignment(off_elems, elem_bytes):
    b = off_elems * elem_bytes
    return 16 if b % 16 == 0 else 8 if b % 8 == 0 else 0


@pytest.mark.parametrize("case", R_CASES)
def test_rejection_case_conditions_paths_and_references(case):
    V, k = case.V, case.k
    race_all = (not case.mask) or case.lp
    assert case.lp == (case.n_top > 0) and (case.form == "logits" or not case.lp)
    assert race_all == (not (case.mask and not case.lp))   # one race per sequence only when masked without logprobs
    for dt in case.dtypes:
        eb = 4 if dt == "f32" else 2
        t_off, t_row, t_seq, d_off, d_row, d_seq = X.rejection_layout(case, dt)
        assert t_row >= V and d_row >= V
        if not case.interleaved:
            for s in range(len(case.seqs)):
                for j in range(k):   # every row of the call is in the class the case names
                    assert _alignment(t_off + s * t_seq + j * t_row, eb) == case.t_align
                    assert _alignment(d_off + s * d_seq + j * d_row, 4) == case.d_align
    for s, q in enumerate(case.seqs):
        where = (case.name, s)
        for dt in case.dtypes:
            assert X.exact_in(q["target"], dt), where
        want = X.ref_rejection(case, s)
        if q["do_sample"]:
            for j in range(k):
                d = int(q["drafts"][j])
                if case.form == "logits":
                    row = q["target"][j]
                    top = row == row.max()
                    assert int(top.sum()) == 1 << q["a"] and np.all(row[~top] - row.max() <= X.ZERO_MASS_BELOW), where
                    p = np.where(top, F32(2.0 ** -q["a"]), F32(0))
                else:
                    p = q["target"][j]
                dd = p.astype(np.float64) - q["draft"][j].astype(np.float64)
                pos_ids = np.nonzero(dd > 0)[0]
                assert set(pos_ids.tolist()) == set(q["recover"]) and np.unique(dd[pos_ids]).size == 1, (where, j)
                assert X._recover_gap(q, j, V) >= X.RACE_MARGIN or len(q["recover"]) == 1, (where, j)
                if not 0 <= d < V:
                    assert not want["accepted"][j], (where, j)
                    continue
                ratio = F32(p[d] / q["draft"][j][d])
                u = X.accept_uniform(q["seed"], q["pos"], j) if case.philox else q["uniform"][j]
                if want["accepted"][j]:     # one fp32 step apart: accepts
                    assert u < ratio and (X.step_up(u) == ratio), (where, j, u, ratio)
                else:                       # equal: rejects
                    assert u == ratio, (where, j, u, ratio)
                assert bool(want["accepted"][j]) == bool(q["accept"][j]), (where, j)
            assert want["accepted_len"] == q["f"] + 1, where
        # ---- the other reference -----------------------------------------------------------------------------------
        o = rref.validate_seq(q["drafts"], q["draft"] if q["do_sample"] else None, q["target"], q["bonus"],
                              do_sample=q["do_sample"], seed=q["seed"], position=q["pos"],
                              uniform=None if case.philox else q["uniform"], target_is_probs=case.form == "probs")
        assert np.array_equal(o["tokens"], want["tokens"]), where
        assert np.array_equal(o["masked"] if case.mask else o["tokens"], want["out"]), where
        assert o["accepted_len"] == want["accepted_len"], where
        if case.lp:
            lps, tops, ids = rref.logprobs_rows(q["target"], want["tokens"], case.n_top)
            assert np.array_equal(ids, want["top_ids"]), where
            np.testing.assert_allclose(lps, want["logprobs"], atol=1e-9)
            np.testing.assert_allclose(tops, want["top_lp"], atol=1e-9)


def test_rejection_axes_are_covered():
    ks = {c.k for c in X.REJECTION}
    assert ks >= {1, 4, 16}
    for k in (4, 16):
        assert {q["f"] for c in X.REJECTION if c.k == k for q in c.seqs} >= {0, k // 2, k - 1, k}
    assert {q["f"] for c in X.REJECTION if c.k == 1 for q in c.seqs} == {0, 1}
    combos = {(c.form, c.mask, c.lp, c.philox) for c in X.REJECTION}
    for mask in (False, True):
        for philox in (False, True):
            assert ("probs", mask, False, philox) in combos
            for lp in (False, True):
                assert ("logits", mask, lp, philox) in combos
    assert {(c.t_align, c.d_align) for c in X.REJECTION} == {(t, d) for t in (16, 8, 0) for d in (16, 8, 0)}
    assert any(c.interleaved for c in X.REJECTION)
    drafts = [int(d) for c in X.REJECTION for q in c.seqs for d in q["drafts"]]
    assert any(d < 0 for d in drafts) and any(d >= 8203 for d in drafts)
    assert any(not q["do_sample"] for c in X.REJECTION for q in c.seqs)
    for V in X.GREEDY_V:
        for row, want in X.greedy_rows(V):
            assert int(np.argmax(row + F32(0))) == want


def _rejection_outputs(case, s, mut):
    with np.errstate(all="ignore"):
        o = X.ref_rejection(case, s, mut)
    return tuple(o["out"].tolist()), o["accepted_len"]


@pytest.mark.parametrize("mut", X.REJECTION_MUTANTS)
def test_every_rejection_mutant_fails_a_case(mut):
    caught = [(c.name, s) for c in X.REJECTION for s in range(len(c.seqs))
              if _rejection_outputs(c, s, mut) != _rejection_outputs(c, s, "")]
    assert caught, mut
    print(mut, "caught by", len(caught), "sequences, e.g.", caught[:3])


def test_the_ratio_search_is_exact():
    for a in (1, 2, 3):
        for r in (0.5, 0.25, 0.3, 0.7001):
            q = X.q_for_ratio(F32(2.0 ** -a), F32(r))
            assert q is None or F32(F32(2.0 ** -a) / q) == F32(r)
