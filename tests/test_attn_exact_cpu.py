"""The exact attention tests without a GPU: every case of tests/attn_exact_cases.py meets the conditions its
exactness rests on, the references return what the construction promises, and a reference with one structural
mistake planted (a mutant: the switch lives here, in a subclass, not in shipped code) breaks a named assertion.

What the GPU test asserts, and which mutant each family catches (test_mutants):
  spike  exact rows equal V[slot(target), kvh] at 0 ulp        decoy  rows aimed outside the visible range match the
  count  every row is c_d / n within 1 ulp                            float64 reference at _check's tolerances
"""
import numpy as np
import pytest

from tests import attn_exact_cases as X
from tests.attn_exact_cases import f64_to_t_bits, t_ulp_distance
from tests.mla_ref import mla_ref

CASES = [pytest.param(c, id=c.name) for c in X.ALL]


def _live(case):
    return sum(case.q_lens)


def _spike_distance(out, want, bits):
    return t_ulp_distance(f64_to_t_bits(out, bits), f64_to_t_bits(want, bits))


# ---- 1. conditions, 2. references agree with the construction ---------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_spike_conditions_and_references(case):
    """Leak condition for every row of every round; the float64 reference, an fp32 restatement with P rounded to T
    before P.V, and the same in 32-key tiles with an online maximum all return V[target] exactly after rounding."""
    _, V = X.caches(case, "spike")
    lay = X.layout(case)
    real = np.abs(V[lay.owner >= 0])
    ratio = float(real.max() / real.min()) if real.size else 1.0
    assert ratio < 2.0
    n = _live(case)
    for r, rnd in enumerate(X.rounds(case)):
        q, want = X.spike_q(case, rnd), X.spike_expect(case, rnd)
        # the inputs are exact in both formats: the kernel sees what the reference sees
        for bits in case.bits:
            assert np.array_equal(X.t_bits_to_f64(f64_to_t_bits(q, bits), bits), q)
        out, leak = X.run_ref(case, q, "spike")
        ex = rnd.exact[:n]
        worst = float((leak[:n][ex]).max()) if ex.any() else 0.0
        assert worst * ratio <= X.LEAK_CAP, (case.name, r, rnd.kind, rnd.place, "leak", worst)
        variants = [("float64", out)]
        for bits in case.bits:
            variants.append((f"fp32, P in {bits}", X.run_ref(case, q, "spike", dtype=np.float32, p_bits=bits)[0]))
            variants.append((f"fp32, P in {bits}, 32-key tiles",
                             X.run_ref(case, q, "spike", dtype=np.float32, p_bits=bits, tile=32)[0]))
        for bits in case.bits:
            want_bits = f64_to_t_bits(want[:n][ex], bits)
            for what, o in variants:
                d = t_ulp_distance(f64_to_t_bits(o[:n][ex], bits), want_bits)
                assert not d.any(), (case.name, r, rnd.kind, what, bits, int(d.max()))
        if not ex.all():   # a decoy must not look like its target: the tolerance compare can tell the two apart
            assert np.abs(out[:n][~ex] - want[:n][~ex]).max(axis=-1).min() > 0.1, (case.name, r, rnd.kind)


@pytest.mark.parametrize("case", CASES)
def test_coverage_condition(case):
    """Every key that some row can see (sequences over 512 keys: every listed edge) is the target of an exact row in
    some round; the diagonal, the window edge and both decoys are there wherever such a key exists."""
    lay = X.layout(case)
    hit = [set() for _ in case.kv_lens]
    kinds = set()
    for rnd in X.rounds(case):
        kinds.add(rnd.kind)
        for b, ql in enumerate(case.q_lens):
            rows = slice(int(lay.q_cu[b]), int(lay.q_cu[b]) + ql)
            t, ex = rnd.target[rows], rnd.exact[rows]
            hit[b] |= set(t[ex & (t >= 0)].tolist())
            for qi in range(ql if case.kv_lens[b] else 0):      # exact targets are visible, decoys are not
                diag = case.kv_lens[b] - ql + qi
                lo = 0 if case.window < 0 else max(0, diag - case.window)
                inside = (t[qi] >= lo) & (t[qi] <= diag)
                assert np.array_equal(inside, ex[qi]), (case.name, rnd.kind, b, qi)
    for b, (ql, kv) in enumerate(zip(case.q_lens, case.kv_lens)):
        if ql == 0 or kv == 0:
            continue
        lo = 0 if case.window < 0 else max(0, kv - ql - case.window)
        seen = set(range(lo, kv))
        must = seen if kv <= X.SMALL_KV else seen & X._edges(case, b, kv, ql)
        assert must <= hit[b], (case.name, b, sorted(must - hit[b])[:8])
        assert {kv - 1, lo} <= hit[b]
    assert {"diag", "edge"} <= kinds
    assert ("decoy diag+1" in kinds) == any(q > 1 for q in case.q_lens)
    assert ("decoy window-1" in kinds) == (case.window >= 0 and any(kv - case.window - 1 > 0 for kv in case.kv_lens))
    if case.kind == "mla":
        assert {r.place for r in X.rounds(case)} == set(X.PLACEMENTS)


@pytest.mark.parametrize("case", [c for c in CASES if X.has_count(c.values[0])])
def test_count_resolution_and_references(case):
    """c_d stays small enough for a single key to show (4 ulps), both references reproduce c_d / n (float64 exactly,
    fp32 with P rounded and tiled within 1 ulp), and one key more, fewer or twice moves some element by >= 4 ulps."""
    n = _live(case)
    want = X.count_expect(case)
    q = np.zeros((n + case.pad_rows, case.heads, case.head_dim + (X.MLA_ROPE if case.kind == "mla" else 0)), np.float32)
    out, _ = X.run_ref(case, q, "count")
    for bits in case.bits:
        assert X.count_max(case) <= X.COUNT_MAX[bits]
        assert not t_ulp_distance(f64_to_t_bits(out, bits), f64_to_t_bits(want, bits)).any()
        o32, _ = X.run_ref(case, q, "count", dtype=np.float32, p_bits=bits, tile=32)
        assert t_ulp_distance(f64_to_t_bits(o32, bits), f64_to_t_bits(want, bits)).max(initial=0) <= 1
    # resolution: one key of a residue class more (a key added or counted twice) or fewer, for every distinct row.
    # Not covered, because no softmax can show it: a key counted twice in a row whose keys are all of its class
    # (n = 1 here: neighbouring keys have different residues), c / n stays 1.
    for c in np.unique(X.count_counts(case)[:n], axis=0):
        if not c.any():
            continue
        present = np.flatnonzero(c)
        classes = {int(present[np.argmax(c[present])]), int(present[np.argmin(c[present])]), int(np.argmin(c))}
        for bits in case.bits:
            base = f64_to_t_bits(c / c.sum(), bits)
            for d in classes:
                for delta in (+1, -1):
                    c2 = c.copy()
                    c2[d] += delta
                    if c2[d] < 0 or c2.sum() == 0 or c[d] == c.sum():
                        continue
                    moved = t_ulp_distance(f64_to_t_bits(c2 / c2.sum(), bits), base).max()
                    assert moved >= 4, (case.name, bits, c.sum(), d, delta, int(moved))


# ---- the semantics are the oracle's, not re-invented ----------------------------------------------------------------
@pytest.mark.parametrize("seed,window,softcap,alibi", [(0, -1, 0.0, False), (1, 10, 0.0, False), (2, -1, 50.0, True),
                                                        (3, 0, 30.0, False), (4, 63, 0.0, True)])
def test_reference_is_pinned_to_the_oracle_on_random_data(seed, window, softcap, alibi):
    from oracle import oracle
    case = X._c(f"pin{seed}", [1, 7, 40, 0, 3], [65, 33, 40, 9, 0], 6, 2, 64, 8, "pin", window=window, softcap=softcap,
                alibi=alibi)
    lay, rng = X.layout(case), np.random.default_rng(seed)
    q = rng.standard_normal((sum(case.q_lens), 6, 64)).astype(np.float32)
    K = rng.standard_normal((lay.n_slots, 2, 64)).astype(np.float32)
    V = rng.standard_normal((lay.n_slots, 2, 64)).astype(np.float32)
    al = X.alibi_of(case)
    got, _ = X.REF(q, K, V, lay, 0.125, softcap, window, al)
    want = oracle.paged_attn(q, K, V, lay.q_cu, lay.kv_cu, lay.bt, lay.bcu, case.block, 0.125, softcap, window, al)
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)
    tiled, _ = X.REF(q, K, V, lay, 0.125, softcap, window, al, tile=32)
    np.testing.assert_allclose(tiled, got, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("name", ["lpr_d64_g2", "window10", "t_w4_d64", "softcap50", "alibi", "mixed", "splits2"])
def test_oracle_agrees_with_the_construction(name):
    from oracle import oracle
    case = X.BY_NAME[name]
    lay, n = X.layout(case), _live(case)
    K, V = X.caches(case, "spike")
    for rnd in X.rounds(case)[:3] + X.rounds(case)[-2:]:
        q, want = X.spike_q(case, rnd), X.spike_expect(case, rnd)
        got = oracle.paged_attn(q[:n], K, V, lay.q_cu, lay.kv_cu, lay.bt, lay.bcu, case.block, X.sm_scale_of(case),
                                case.softcap, case.window, X.alibi_of(case))
        ex = rnd.exact[:n]
        assert not _spike_distance(got, want[:n], "f16")[ex].any(), (name, rnd.kind)
    if X.has_count(case):
        Kc, Vc = X.caches(case, "count")
        got = oracle.paged_attn(np.zeros((n, case.heads, case.head_dim), np.float32), Kc, Vc, lay.q_cu, lay.kv_cu, lay.bt,
                                lay.bcu, case.block, X.sm_scale_of(case), case.softcap, case.window, None)
        assert _spike_distance(got, X.count_expect(case)[:n], "f16").max(initial=0) <= 1


@pytest.mark.parametrize("name", ["mla_d512_h8", "mla_prefill_s2", "mla_decode_b5"])
def test_mla_reference_is_pinned_to_mla_ref(name):
    case = X.BY_NAME[name]
    lay, D = X.layout(case), case.head_dim
    rng = np.random.default_rng(len(name))
    n = _live(case)
    q = rng.standard_normal((n, case.heads, D + X.MLA_ROPE))
    kv, kr = rng.standard_normal((lay.n_slots, D)), rng.standard_normal((lay.n_slots, X.MLA_ROPE))
    got, _ = X.REF(q, np.concatenate([kv, kr], 1)[:, None], kv[:, None], lay, 0.05)
    want = mla_ref(q[..., :D], q[..., D:], kv, kr, lay.q_cu, lay.kv_cu, lay.bt, lay.bcu, case.block, 0.05)
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-12)


# ---- 3. mutants ---------------------------------------------------------------------------------------------------
def _mutant(**methods):
    return type("Mutant", (X.AttnRef,), methods)()


def _vis(shift_diag=0, shift_window=0, drop=None, past_end=False):
    def visible(self, q_len, kv_len, n_alloc, window):
        j = np.arange(n_alloc)[None, :]
        diag = (kv_len - q_len + np.arange(q_len))[:, None]
        vis = (j <= diag + shift_diag) & (j < kv_len)
        if past_end:                                    # the row that sees the last key also takes the one after it
            vis |= (j == kv_len) & (diag == kv_len - 1)
        if window >= 0:
            vis &= (diag - j) <= window + shift_window
        if drop is not None:
            vis &= ~drop(j, kv_len)
        return vis
    return visible


def _share_start(weight):
    def times(self, kv_len, n_alloc):
        t = np.ones(n_alloc)
        t[-(-kv_len // 2)] = weight                     # the first key of the second of two shares
        return t
    return times


def _next_block(self, b, lay):
    idx = np.minimum(np.arange(lay.bcu[b], lay.bcu[b + 1]) + 1, len(lay.bt) - 1)
    return (lay.bt[idx].astype(np.int64)[:, None] + np.arange(lay.block)[None, :]).reshape(-1)


def _half_offset(self, b, lay):
    first = lay.bt[lay.bcu[b]:lay.bcu[b + 1]].astype(np.int64)
    return (first[:, None] + (np.arange(lay.block) % max(lay.block // 2, 1))[None, :]).reshape(-1)


def _drop_columns(lo_of, hi_of):
    def key_columns(self, dk):
        m = np.ones(dk)
        m[lo_of(dk):hi_of(dk)] = 0
        return m
    return key_columns


# (number in the issue's table, what, mutant, cases to try, families that must catch it, families that cannot)
MUTANTS = [
    (1, "diagonal + 1", _mutant(visible=_vis(shift_diag=1)), ["t_w4_d64"], {"count", "decoy"}, set()),
    (2, "diagonal - 1", _mutant(visible=_vis(shift_diag=-1)), ["t_w4_d64", "lpr_d64_g2"], {"spike", "count"}, set()),
    (3, "window edge + 1", _mutant(visible=_vis(shift_window=1)), ["window10"], {"count", "decoy"}, set()),
    (3, "window edge - 1", _mutant(visible=_vis(shift_window=-1)), ["window10"], {"spike", "count"}, set()),
    (4, "last key of the sequence dropped", _mutant(visible=_vis(drop=lambda j, kv: j == kv - 1)), ["lpr_d64_g2"],
     {"spike", "count"}, set()),
    (5, "keys with j % 64 == 63 dropped", _mutant(visible=_vis(drop=lambda j, kv: j % 64 == 63)), ["nw1"],
     {"spike", "count"}, set()),
    (6, "first key of a share dropped", _mutant(times=_share_start(0.0)), ["splits2"], {"spike", "count"}, set()),
    # the spike family cannot see a key counted twice: 2 V / (2 + leak) rounds to V.  Only the count family does.
    (7, "first key of a share counted twice", _mutant(times=_share_start(2.0)), ["splits2"], {"count"}, {"spike"}),
    (8, "key kv_len included", _mutant(visible=_vis(past_end=True)), ["lpr_d64_g2"], {"count", "spike"}, set()),
    (9, "block index + 1", _mutant(alloc_slots=_next_block), ["lpr_d64_g2"], {"spike"}, set()),
    (10, "in-block offset taken mod block / 2", _mutant(alloc_slots=_half_offset), ["lpr_d64_g2"], {"spike"}, set()),
    (11, "kvh = h % n_kv", _mutant(kv_head=lambda self, h, group, n_kv: h % n_kv), ["lpr_d64_g2"], {"spike"}, set()),
    (12, "output columns rotated by 8", _mutant(finish=lambda self, o: np.roll(o, 8, axis=1)), ["lpr_d64_g2"],
     {"spike", "count"}, set()),
    (13, "MLA: RoPE part dropped", _mutant(key_columns=_drop_columns(lambda dk: dk - 64, lambda dk: dk)), ["mla_d512_h8"],
     {"spike:rope"}, {"spike:all", "count"}),
] + [
    (14, f"MLA: contraction quarter {w} dropped",
     _mutant(key_columns=_drop_columns(lambda dk, w=w: w * dk // 4, lambda dk, w=w: (w + 1) * dk // 4)), ["mla_d512_h8"],
     {f"spike:q{w}"}, {"count"} | {f"spike:q{v}" for v in range(4) if v != w})
    for w in range(4)
]


def _caught(case, ref, bits="bf16"):
    """the assertions of the GPU test that fail when the device computes what `ref` computes"""
    n, found = _live(case), set()
    for rnd in X.rounds(case):
        q, want = X.spike_q(case, rnd), X.spike_expect(case, rnd)
        out, _ = X.run_ref(case, q, "spike", ref)
        ex = rnd.exact[:n]
        if _spike_distance(out[:n], want[:n], bits)[ex].any():
            found |= {"spike", f"spike:{rnd.place}"}
        if not ex.all():
            true, _ = X.run_ref(case, q, "spike")
            if not np.allclose(out[:n][~ex], true[:n][~ex], rtol=1e-2, atol=1e-2):
                found.add("decoy")
    if X.has_count(case):
        q0 = np.zeros((n, case.heads, X.caches(case, "count")[0].shape[2]), np.float32)
        out, _ = X.run_ref(case, q0, "count", ref)
        if t_ulp_distance(f64_to_t_bits(out, bits), f64_to_t_bits(X.count_expect(case)[:n], bits)).max(initial=0) > 1:
            found.add("count")
    return found


@pytest.mark.parametrize("number,what,ref,names,must,cannot", MUTANTS, ids=[f"{m[0]}-{m[1]}" for m in MUTANTS])
def test_mutants(number, what, ref, names, must, cannot):
    """A mutant that no case catches means a case is missing from the tables."""
    found = set()
    for name in names:
        found |= _caught(X.BY_NAME[name], ref)
    assert must <= found, (what, "not caught by", sorted(must - found))
    assert not (cannot & found), (what, "unexpectedly caught by", sorted(cannot & found))


def test_the_unmutated_reference_passes_every_assertion():
    for name in sorted({n for m in MUTANTS for n in m[3]}):
        assert not _caught(X.BY_NAME[name], X.REF), name
