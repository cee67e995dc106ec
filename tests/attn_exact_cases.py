"""References, input builders and case tables of the exact structural tests of the attention kernels (attn.hip,
attn_tile.hip, mla.hip): what tests/test_attn_exact_gpu.py runs on the device and what tests/test_attn_exact_cpu.py
checks the conditions, the references and the mutants on without one.  Imports no GPU code.

Semantics (oracle/slm_oracle.c, oracle_paged_attn; pinned against it by the CPU test): query head h reads KV head
kvh = h // G; query token qi of a sequence has diag = kv_len - q_len + qi; key j is visible iff j <= diag and
(window < 0 or diag - j <= window); a score is sm_scale q.k, then soft-capped cap tanh(s / cap), then + slope_h j;
a row that sees nothing is zero.  Key j of sequence b lives in slot table[bcu[b] + j // block] + j % block.  MLA
(tests/mla_ref.py) is the same with ONE KV head whose key is [latent | rope] and whose value is the latent.

Two input families, both built from the case's name as the seed:

  spike  K rows are random +-1 codes, V rows random values exact in both 16-bit formats with |v| in [1, 2).  The
         query of a row is the code of ONE target key, sm_scale a power of two (64 / head_dim): the target scores 64,
         every other key a random walk far below.  The target's weight is exp(0) = 1 in every softmax order (also
         with the tile kernels' lazy rescale: the spike exceeds their threshold), the others add up to `leak`, and
         with leak max|V| / min|V| <= 2^-14 -- a quarter of f16's half ulp; a condition on the table, asserted on the
         CPU for every row -- the output IS V[slot(target), kvh] bit for bit.  Rounds re-target the rows over one
         cache until every key of every sequence was a target (sequences over 512 keys: the listed edges); decoy
         rounds aim one step OUTSIDE the visible range, where the row must see mismatches only (compared with the
         float64 reference at test_attention_gpu.py's tolerances).
  count  q = 0: every visible weight is 1 exactly; V[slot(j), kvh, d] = (d == j mod D).  out[r, d] = c_d / n, the
         number of visible keys of residue d over the number of visible keys: small integers, exact in fp32 in any
         order, one rounding at the end: <= 1 ulp of T.  With c_d <= 64 (bf16) / 256 (f16) a key dropped, added or
         counted twice moves some element by >= 4 ulps.

Poison: slots no sequence owns and the tail of every last block hold the code of that sequence's last key and
V = 256 (finite on purpose: 0 * NaN inside an MFMA would poison a correct kernel).

Worst distance on an MI355X (gfx950) over all cases and both dtypes: spike 0 ulp, count 0 ulp (MEASURED below).
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

from tests import helpers
from tests.glue_ref import f64_to_t_bits, t_bits_to_f64, t_ulp_distance  # noqa: F401  (re-exported to the tests)

BITS = ("bf16", "f16")
POISON_V = 256.0
LEAK_CAP = 2.0 ** -14
COUNT_MAX = {"bf16": 64, "f16": 256}      # largest c_d at which one key still moves an element by 4 ulps
SMALL_KV = 512                            # up to here every key is a target; above, the edges listed in _edges()
MLA_ROPE = 64
PLACEMENTS = ("all", "rope", "q0", "q1", "q2", "q3")     # MLA: which columns of the 576-wide contraction carry the code

# kind "mha" | "mla"; knobs: (name, value) pairs the test sets through tune(...); ws: None, or whether the workspace
# query must answer > 0 (partials + a combine pass); splits: None, or what the split-count query must answer;
# path: the rule of plan_attn / launch_attn_tile / mla_* that routes the case
Case = namedtuple("Case", "name kind q_lens kv_lens heads kv_heads head_dim block window softcap alibi num_splits "
                          "knobs max_kv_hint strided pad_rows bits ws splits path")


def _c(name, q_lens, kv_lens, heads, kv_heads, head_dim, block, path, kind="mha", window=-1, softcap=0.0, alibi=False,
       num_splits=0, max_kv_hint=None, strided=False, pad_rows=0, bits=BITS, ws=None, splits=None, **knobs):
    if isinstance(q_lens, int):
        q_lens = [q_lens] * len(kv_lens)
    assert len(q_lens) == len(kv_lens) and all(q <= k or q == 0 or k == 0 for q, k in zip(q_lens, kv_lens)), name
    return Case(name, kind, tuple(q_lens), tuple(kv_lens), heads, kv_heads, head_dim, block, window, softcap, alibi,
                num_splits, tuple(sorted(knobs.items())), max_kv_hint, strided, pad_rows, bits, ws,
                num_splits if num_splits > 0 and splits is None and kind == "mha" else splits, path)


def _rng(name, stream):
    return np.random.default_rng([zlib.crc32(name.encode()), stream])


def sm_scale_of(case):
    """a power of two per head_dim: the target scores 64 (MLA: 72 ... 96 over all 576 / 320 / 192 columns)"""
    if case.kind == "mla":
        return 2.0 ** -int(np.floor(np.log2((case.head_dim + MLA_ROPE) / 64)))
    return 64.0 / case.head_dim


def alibi_of(case):
    """slopes with slope * kv_len <= 4: the spike stays the row's maximum by a wide margin"""
    if not case.alibi:
        return None
    return (4.0 / max(max(case.kv_lens), 1) * (np.arange(case.heads) + 1) / case.heads).astype(np.float32)


# ---- the float64 reference --------------------------------------------------------------------------------------
class AttnRef:
    """Paged varlen GQA attention with soft-cap, alibi and sliding window; K and V may differ in width (MLA).  The
    methods below are the semantics; the mutants of the CPU test override one each.

    dtype: the arithmetic (float64, or float32 for the restatement of what a kernel does); p_bits: round P to that
    16-bit format before P.V, as every MFMA kernel does; tile: process the keys in tiles of that many with an
    online maximum.  Returns (out [T, H, Dv], leak [T, H]): leak = sum of exp(s - max) over the visible keys
    other than the maximum."""

    def kv_head(self, h, group, n_kv):
        return h // group

    def alloc_slots(self, b, lay):
        """slots of every position of sequence b's blocks, the tail of the last block included"""
        first = lay.bt[lay.bcu[b]:lay.bcu[b + 1]].astype(np.int64)
        return (first[:, None] + np.arange(lay.block)[None, :]).reshape(-1)

    def visible(self, q_len, kv_len, n_alloc, window):
        j = np.arange(n_alloc)[None, :]
        diag = (kv_len - q_len + np.arange(q_len))[:, None]
        vis = (j <= diag) & (j < kv_len)
        if window >= 0:
            vis &= (diag - j) <= window
        return vis

    def times(self, kv_len, n_alloc):
        """how often each key enters the sums (a correct kernel: once)"""
        return np.ones(n_alloc)

    def key_columns(self, dk):
        return np.ones(dk)

    def finish(self, o):
        return o

    def __call__(self, q, kc, vc, lay, sm_scale, softcap=0.0, window=-1, alibi=None, dtype=np.float64, p_bits=None,
                 tile=None):
        f = dtype
        q, kc, vc = np.asarray(q, f), np.asarray(kc, f), np.asarray(vc, f)
        T, H, _ = q.shape
        n_kv, dv = kc.shape[1], vc.shape[2]
        G = H // n_kv
        out = np.zeros((T, H, dv), f)
        leak = np.zeros((T, H))
        cols = self.key_columns(kc.shape[2]).astype(f)
        for b in range(len(lay.q_lens)):
            q_len, kv_len, q0 = lay.q_lens[b], lay.kv_lens[b], int(lay.q_cu[b])
            if q_len == 0 or kv_len == 0:
                continue
            slots = self.alloc_slots(b, lay)
            vis = self.visible(q_len, kv_len, len(slots), window)
            mult = self.times(kv_len, len(slots)).astype(f)
            by_kvh = {}
            for h in range(H):
                by_kvh.setdefault(self.kv_head(h, G, n_kv), []).append(h)
            for kvh, hs in by_kvh.items():                  # rows (token, head) of the heads that share a KV head
                k, v = kc[slots, kvh] * cols, vc[slots, kvh]
                s = (q[q0:q0 + q_len, hs].reshape(q_len * len(hs), -1) @ k.T) * f(sm_scale)
                if softcap > 0:
                    s = np.tanh(s / f(softcap)) * f(softcap)
                if alibi is not None:
                    s = s + np.tile(np.asarray(alibi, f)[hs], q_len)[:, None] * np.arange(len(slots), dtype=f)[None, :]
                s = np.where(np.repeat(vis, len(hs), axis=0), s, -np.inf)
                o, lk = self._softmax_pv(s, v, mult, f, p_bits, tile)
                out[q0:q0 + q_len, hs] = self.finish(o).reshape(q_len, len(hs), dv)
                leak[q0:q0 + q_len, hs] = lk.reshape(q_len, len(hs))
        return out, leak

    @staticmethod
    def _round_p(p, p_bits):
        if p_bits is None:
            return p
        if p.dtype == np.float32:                           # one rounding, fp32 -> T
            return helpers._from_t_bits(helpers._t_bits(p, p_bits), p_bits)
        return t_bits_to_f64(f64_to_t_bits(p, p_bits), p_bits)

    def _softmax_pv(self, s, v, mult, f, p_bits, tile):
        rows, n = s.shape
        step = n if tile is None else tile
        m = np.full((rows, 1), -np.inf, f)
        den = np.zeros((rows, 1), f)
        o = np.zeros((rows, v.shape[1]), f)
        for t0 in range(0, n, step):
            st = s[:, t0:t0 + step]
            m_new = np.maximum(m, st.max(axis=1, keepdims=True))
            safe = np.where(np.isfinite(m_new), m_new, f(0))
            with np.errstate(invalid="ignore"):
                scale = np.where(np.isfinite(m), np.exp(m - safe), f(0)).astype(f)
            p = (np.exp(st - safe) * mult[None, t0:t0 + step]).astype(f)
            den = den * scale + p.sum(axis=1, keepdims=True, dtype=f)
            o = o * scale + (self._round_p(p, p_bits) @ v[t0:t0 + step]).astype(f)
            m = m_new
        live = den[:, 0] > 0
        o = np.where(live[:, None], o / np.where(live[:, None], den, f(1)), f(0))
        # everything but the maximum (one key of weight exp(0) = 1)
        return o, np.where(live, den[:, 0].astype(np.float64) - 1.0, 0.0)


REF = AttnRef()


# ---- layout, caches, rounds -------------------------------------------------------------------------------------
Layout = namedtuple("Layout", "q_lens kv_lens q_cu kv_cu bt bcu block n_slots owner key_of")
Round = namedtuple("Round", "kind target exact place")   # target [T, H] key index (-1: the row sees nothing);
                                                           # exact [T, H]: the row owes V[target] (False: decoy)


@functools.lru_cache(maxsize=None)
def layout(case):
    """Shuffled, non-contiguous block table with two blocks that nobody owns."""
    B = case.block
    nblk = [(k + B - 1) // B for k in case.kv_lens]
    ids = _rng(case.name, 1).permutation(sum(nblk) + 2)
    bt = (ids[:sum(nblk)] * B).astype(np.int32)
    bcu = np.concatenate([[0], np.cumsum(nblk)]).astype(np.int32)
    n_slots = (sum(nblk) + 2) * B
    owner, key_of = np.full(n_slots, -1), np.full(n_slots, -1)
    for b, kv in enumerate(case.kv_lens):
        alloc = (bt[bcu[b]:bcu[b + 1]].astype(np.int64)[:, None] + np.arange(B)[None, :]).reshape(-1)
        owner[alloc[:kv]], key_of[alloc[:kv]] = b, np.arange(kv)
        owner[alloc[kv:]] = -2 - b                         # tail of b's last block: poison that belongs to b
    cu = lambda a: np.concatenate([[0], np.cumsum(a)]).astype(np.int32)  # noqa: E731
    return Layout(case.q_lens, case.kv_lens, cu(case.q_lens), cu(case.kv_lens), bt, bcu, B, n_slots, owner, key_of)


def slot_of(lay, b, j):
    j = np.asarray(j)
    return lay.bt[lay.bcu[b] + j // lay.block].astype(np.int64) + j % lay.block


@functools.lru_cache(maxsize=None)
def caches(case, family):
    """(K [S, HKV, Dk], V [S, HKV, Dv]) as float32, every value exact in bf16 and f16."""
    lay, rng = layout(case), _rng(case.name, 2)
    S, D = lay.n_slots, case.head_dim
    mla = case.kind == "mla"
    n_kv = 1 if mla else case.kv_heads
    sign = lambda *shape: rng.integers(0, 2, size=shape).astype(np.float32) * 2 - 1  # noqa: E731
    K = sign(S, n_kv, D)
    if family == "count":
        V = np.zeros((S, n_kv, D), np.float32)
        own = np.flatnonzero(lay.owner >= 0)
        V[own, :, lay.key_of[own] % D] = 1.0
    elif mla:
        V = K.copy()
    else:
        V = sign(S, n_kv, D) * (1 + rng.integers(0, 128, size=(S, n_kv, D)).astype(np.float32) / 128)
    rope = sign(S, 1, MLA_ROPE) if mla else None
    # poison: the code of the owner's last key (slots nobody owns: of the first sequence that has one)
    donors = [b for b, kv in enumerate(lay.kv_lens) if kv > 0]
    for s in np.flatnonzero(lay.owner < 0):
        b = -2 - lay.owner[s] if lay.owner[s] <= -2 else (donors[0] if donors else None)
        src = None if b is None else slot_of(lay, b, lay.kv_lens[b] - 1)
        if src is not None:
            K[s] = K[src]
            if mla:
                rope[s] = rope[src]
        V[s] = POISON_V * K[s] if (mla and family == "spike") else POISON_V
    if mla:
        K = np.concatenate([V, rope], axis=2)              # the latent row is K and V at once
    return K, V


def _cdiv(a, b):
    return -(-a // b)


def _edges(case, b, kv_len, q_len):
    """the listed targets of a long sequence"""
    e = {0, kv_len - 1}
    for qi in range(q_len):
        diag = kv_len - q_len + qi
        e |= {diag} | ({diag - case.window} if case.window >= 0 else set())
    for m in range(0, kv_len + 32, 32):
        e |= {m - 1, m, m + 1}
    for m in range(0, kv_len + case.block, case.block):
        e |= {m - 1, m}
    for shares in (2, 3, 4, 7, 8):                          # the first key of a split-KV share, whole or in 64-key units
        for per in (_cdiv(kv_len, shares), _cdiv(_cdiv(kv_len, 64), shares) * 64):
            e |= {s * per + d for s in range(1, shares) for d in (-1, 0, 1)}
    return {j for j in e if 0 <= j < kv_len}


def _window_lo(case, diag):
    return 0 if case.window < 0 else max(0, diag - case.window)


@functools.lru_cache(maxsize=None)
def rounds(case):
    """Rounds of targets: the diagonal, the left edge of the visible range, then greedy rounds (every row takes the
    largest key it sees that was no target yet) until every required key was one, then the decoys."""
    lay = layout(case)
    T, H = sum(case.q_lens) + case.pad_rows, case.heads
    rng = _rng(case.name, 3)
    need = []
    for b, (ql, kv) in enumerate(zip(case.q_lens, case.kv_lens)):
        if ql == 0 or kv == 0:
            need.append(set())
            continue
        seen = set(range(_window_lo(case, kv - ql), kv))    # the union of the rows' visible ranges
        need.append(seen if kv <= SMALL_KV else seen & _edges(case, b, kv, ql))
    out = []

    def make(kind, pick, place="all"):
        tgt, exact = np.full((T, H), -1), np.ones((T, H), bool)
        for b, (ql, kv) in enumerate(zip(case.q_lens, case.kv_lens)):
            if kv == 0:
                continue
            for qi in range(ql):
                diag = kv - ql + qi
                t, ex = pick(b, qi, _window_lo(case, diag), diag, kv)
                tgt[lay.q_cu[b] + qi], exact[lay.q_cu[b] + qi] = t, ex
                need[b] -= set(np.asarray(t)[np.asarray(ex)].tolist())
        out.append(Round(kind, tgt, exact, place))

    def greedy(b, qi, lo, diag, kv):
        todo = sorted((j for j in need[b] if lo <= j <= diag), reverse=True)[:H]
        rest = lo + rng.integers(0, diag - lo + 1, size=H - len(todo))
        return np.concatenate([np.asarray(todo, np.int64), rest]), np.ones(H, bool)

    # MLA: the rounds take the code placements in turn (at least one round each)
    place = lambda: PLACEMENTS[len(out) % len(PLACEMENTS)] if case.kind == "mla" else "all"  # noqa: E731
    make("diag", lambda b, qi, lo, diag, kv: (np.full(H, diag), np.ones(H, bool)), place())
    make("edge", lambda b, qi, lo, diag, kv: (np.full(H, lo), np.ones(H, bool)), place())
    while any(need) or (case.kind == "mla" and len(out) < len(PLACEMENTS)):
        assert len(out) < 200, (case.name, "the rows cannot reach every key in 200 rounds")
        make("cover", greedy, place())
    if any(ql > 1 for ql in case.q_lens):                   # one past the diagonal
        make("decoy diag+1", lambda b, qi, lo, diag, kv:
             (np.full(H, diag + 1), np.zeros(H, bool)) if diag + 1 < kv else (np.full(H, diag), np.ones(H, bool)))
    if case.window >= 0 and any(kv - case.window - 1 > 0 for kv in case.kv_lens):   # one before the window
        make("decoy window-1", lambda b, qi, lo, diag, kv:
             (np.full(H, lo - 1), np.zeros(H, bool)) if lo > 0 else (np.full(H, diag), np.ones(H, bool)))
    return out


def placement_columns(case, place):
    """(mask over the [latent | rope] columns, power-of-two query scale that lifts the target score to >= 64)"""
    dk = case.head_dim + (MLA_ROPE if case.kind == "mla" else 0)
    mask = np.zeros(dk, np.float32)
    if place == "all":
        mask[:] = 1
    elif place == "rope":
        mask[case.head_dim:] = 1
    else:                                                   # wave w of mla_kernel takes k-steps [w NSUB/4, (w+1) NSUB/4)
        w = int(place[1])
        mask[w * dk // 4:(w + 1) * dk // 4] = 1
    scale = 2.0 ** int(np.ceil(np.log2(64.0 / (sm_scale_of(case) * mask.sum()))))
    return mask, max(scale, 1.0)


def spike_q(case, rnd):
    """q [T, H, Dk] of one round: the (scaled, masked) code of each row's target; rows that see nothing and padding
    rows get the code of slot 0"""
    lay = layout(case)
    K, _ = caches(case, "spike")
    n_kv = K.shape[1]
    G = case.heads // n_kv
    T, H = rnd.target.shape
    q = np.broadcast_to(K[0, (np.arange(H) // G)], (T, H, K.shape[2])).copy()
    for b, ql in enumerate(case.q_lens):
        for qi in range(ql):
            t = lay.q_cu[b] + qi
            if rnd.target[t, 0] >= 0:
                q[t] = K[slot_of(lay, b, rnd.target[t]), np.arange(H) // G]
    mask, scale = placement_columns(case, rnd.place)
    return q * mask * scale


def spike_expect(case, rnd):
    """float32 [T, H, Dv]: V[slot(target), kvh] for the exact rows, 0 for rows that see nothing; decoy and padding
    rows are not covered (rnd.exact is False / the row is past q_cu[-1])"""
    lay = layout(case)
    _, V = caches(case, "spike")
    G = case.heads // V.shape[1]
    T, H = rnd.target.shape
    want = np.zeros((T, H, V.shape[2]), np.float32)
    for b, ql in enumerate(case.q_lens):
        for qi in range(ql):
            t = lay.q_cu[b] + qi
            if rnd.target[t, 0] >= 0:
                want[t] = V[slot_of(lay, b, rnd.target[t]), np.arange(H) // G]
    return want


def count_counts(case):
    """int [T, D]: c_d of every token row, from the visibility rule alone (no softmax)"""
    lay, D = layout(case), case.head_dim
    c = np.zeros((sum(case.q_lens) + case.pad_rows, D), np.int64)
    for b, (ql, kv) in enumerate(zip(case.q_lens, case.kv_lens)):
        for qi in range(ql if kv else 0):
            diag = kv - ql + qi
            c[lay.q_cu[b] + qi] = np.bincount(np.arange(_window_lo(case, diag), diag + 1) % D, minlength=D)
    return c


def count_expect(case):
    """float64 [T, H, D]: c_d / n, zero for rows that see nothing"""
    c = count_counts(case)
    n = c.sum(axis=1, keepdims=True)
    want = np.where(n > 0, c / np.maximum(n, 1), 0.0)
    return np.broadcast_to(want[:, None, :], (c.shape[0], case.heads, c.shape[1])).copy()


def count_max(case):
    return max((-(-kv // case.head_dim) for kv in case.kv_lens), default=0)


def run_ref(case, q, family, ref=REF, **kw):
    K, V = caches(case, family)
    return ref(q, K, V, layout(case), sm_scale_of(case), case.softcap, case.window,
               alibi_of(case) if family == "spike" else None, **kw)


def has_count(case):
    return not case.alibi                                   # the count family has no alibi: every weight is 1


# ---- case tables ------------------------------------------------------------------------------------------------
# Stream (token) kernel: max_q_len = 1, and either G < 8 or fewer than 64 (sequence, KV head) pairs keeps the rows off
# the tile kernel (decode_on_tile).  Without a knob: n_tokens < 16 => no balanced partition, max_kv_len <= 129 =>
# max_by_len <= 2 splits.
STREAM = []
for _d, _blk in ((32, 1), (64, 8), (128, 16), (256, 256)):
    for _g in (1, 2, 4, 8):
        # plan_attn: lpr = 4 / 8 / 16 / 32 by head_dim, gc = G; batch 3 x 2 KV heads = 6 pairs < 64
        STREAM.append(_c(f"lpr_d{_d}_g{_g}", 1, [33, 1 if _g in (1, 4) else 0, 65], 2 * _g, 2, _d, _blk,
                         f"token kernel LPR {_d // 8} GC {_g}",
                         ws=False, splits=1, SLM_ATTN_W=1))
for _g in (1, 2, 4):
    for _w in (1, 2):
        # plan_attn: SLM_ATTN_W forces the one- / two-chunk form at head_dim 128, gc <= 4, no soft-cap / alibi
        STREAM.append(_c(f"w{_w}_g{_g}", 1, [63, 32, 65], 2 * _g, 2, 128, 16, f"token kernel W = {_w}", SLM_ATTN_W=_w))
_L130 = [(0, 1, 31, 32, 33)[i % 5] for i in range(130)]
for _w in (1, 2):
    # plan_attn: n_tokens > 128 keeps hpw = hpw_max (4 KV heads per wave load at LPR 16, 8 at W = 2's LPR 8)
    STREAM.append(_c(f"wide_load_w{_w}", 1, _L130, 8, 8, 128, 8, f"token kernel, {4 * _w} KV heads per wave load",
                     ws=False, SLM_ATTN_W=_w))
for _nw in (1, 2, 8):
    STREAM.append(_c(f"nw{_nw}", 1, [65, 0, 33], 8, 2, 128, 8, f"token kernel, {_nw} waves", SLM_ATTN_NW=_nw, SLM_ATTN_W=1))
for _k, _v in (("U", 2), ("U", 4), ("NT", 0), ("NT", 1)):
    STREAM.append(_c(f"{_k.lower()}{_v}", 1, [65, 0, 33], 8, 2, 128, 8, f"token kernel, SLM_ATTN_{_k} = {_v}",
                     **{f"SLM_ATTN_{_k}": _v, "SLM_ATTN_W": 1}))
for _s in (2, 3, 7):
    # num_splits > 0: forced_splits, classic per-sequence shares + combine; the 5-key sequence leaves shares empty
    STREAM.append(_c(f"splits{_s}", 1, [5, 64, 129, 700], 8, 2, 128, 16, f"classic split-KV, {_s} shares", num_splits=_s,
                     ws=True))
STREAM.append(_c("splits3_window10", 1, [5, 64, 129, 300], 8, 2, 128, 16, "classic split-KV over a window", num_splits=3,
                 window=10, ws=True))
# SLM_ATTN_BAL = 2: bal_mode == 2 takes the balanced partition below its batch floor too (q_len 1, no window, no
# forced split, n_tokens == batch); it always has partial slots => workspace
STREAM += [
    _c("bal_b3_blk8", 1, [129, 0, 300], 8, 2, 128, 8, "balanced partition, batch 3", ws=True, SLM_ATTN_BAL=2),
    _c("bal_b20_blk16", 1, [(0, 1, 31, 64, 65, 127, 128, 129, 200, 33)[i % 10] for i in range(20)], 8, 2, 128, 16,
       "balanced partition, batch 20, ragged", ws=True, SLM_ATTN_BAL=2),
    _c("bal_b20_w2", 1, [(64, 1, 0, 300, 33, 129, 128, 63, 200, 31)[i % 10] for i in range(20)], 8, 4, 128, 8,
       "balanced partition, two-chunk form", ws=True, SLM_ATTN_BAL=2, SLM_ATTN_W=2),
    # bal_qmin comes from the hint: the 700-key sequence needs more pieces than slots and is streamed whole
    _c("bal_hint64", 1, [700, 1, 64], 8, 2, 128, 16, "balanced partition, max_kv_len understated", max_kv_hint=64,
       ws=True, SLM_ATTN_BAL=2),
]
for _win in (0, 1, 10, 63, 64):
    # max_kv_len 65 => max_by_len 1: one pass; 129 => two shares (each clipped by the window) + combine
    _long = _win in (1, 63)
    STREAM.append(_c(f"window{_win}", 1, [65, 1, 129 if _long else 33], 8, 2, 128, 16,
                     "token kernel, sliding window, " + ("two shares" if _long else "one pass"), window=_win,
                     pad_rows=2, ws=_long, splits=2 if _long else 1))
STREAM += [
    # launch_token_kernel: soft-cap or alibi => the SC instantiation (U 2, no non-temporal loads)
    _c("softcap50", 1, [65, 33, 129], 8, 2, 128, 16, "token kernel, SC instantiation (soft-cap)", softcap=50.0),
    _c("softcap50_d256", 1, [65, 33, 129], 4, 2, 256, 16, "token kernel, SC instantiation (soft-cap)", softcap=50.0),
    _c("alibi", 1, [65, 33, 129], 8, 2, 128, 16, "token kernel, SC instantiation (alibi)", alibi=True),
    _c("alibi_d64", 1, [65, 33, 129], 8, 2, 64, 8, "token kernel, SC instantiation (alibi)", alibi=True),
    _c("strided", 1, [65, 33, 129], 8, 2, 128, 16, "token kernel, strided q / out views", strided=True, pad_rows=2),
]

# Tile kernel: max_q_len > 1 and no forced split (slm_paged_kv_varlen_mha); launch_attn_tile: nw = ceil(rows / 32)
# with rows = max q_len * G, 3 -> 4.  Row classes per sequence on the device: rows <= 32 one-wave tiles, above that
# the 2- / 4-wave launch.
TILE = []
for _d in (64, 128):
    TILE += [
        _c(f"t_w1_d{_d}", [8, 5], [8, 65], 8, 2, _d, 16, "tile kernel, one wave (rows 32, 20)"),
        _c(f"t_w2_d{_d}", [16, 9], [16, 65], 8, 2, _d, 16, "tile kernel, two waves (rows 64, 36)"),
        _c(f"t_w4_d{_d}", [33, 17, 64], [33, 129, 64], 8, 2, _d, 16, "tile kernel, four waves (rows 132, 68, 256), two shares",
           ws=True, splits=2),
        # G = 3, q_len 30: a 32-row tile holds tokens with different causal limits
        _c(f"t_g3_d{_d}", [30, 30], [30, 127], 6, 2, _d, 8, "tile kernel, group 3: mixed causal limits in a row tile"),
    ]
for _pf in (None, 5, 4, 2, 0):
    for _feat, _kw in (("plain", {}), ("window", dict(window=63)), ("softcap", dict(softcap=50.0))):
        _k = {} if _pf is None else dict(SLM_ATTN_TILE_PF=_pf)
        # launch_attn_tile: pf_mode picks LDS-DMA + pipeline (default, plain only) / 5 DMA alone / 4 register-staged
        # 64-row tiles / 2 32-row single buffer / 0 no prefetch; q_len 5 and 1 ride along on the one-wave class and
        # the token kernel
        # max_kv_len 127 => max_by_len 1: no split; the windowed form runs with the call's two shares (129 keys)
        _n = 129 if _feat == "window" else 127
        TILE.append(_c(f"pf{'def' if _pf is None else _pf}_{_feat}", [65, 33, 5, 1], [_n, 33, 64, 31], 8, 2, 128, 16,
                       f"tile staging form {_pf}, {_feat}", ws=_n == 129, splits=_n // 64, **_kw, **_k))
    TILE.append(_c(f"pf{'def' if _pf is None else _pf}_d64", [65, 33, 5, 1], [127, 33, 64, 31], 8, 2, 64, 16,
                   f"tile staging form {_pf}, head_dim 64", ws=False, splits=1,
                   **({} if _pf is None else dict(SLM_ATTN_TILE_PF=_pf))))
for _kv2 in (0, 1):
    # launch_attn_tile: kv2 exists for plain, DMA, pipeline, 4 waves, head_dim 128; 1 / 2 / 3 / 4 64-key tiles
    TILE.append(_c(f"kv2_{_kv2}", [64, 128, 129, 33], [64, 128, 129, 200], 8, 2, 128, 16,
                   f"tile kernel, SLM_ATTN_TILE_KV2 = {_kv2}, 1 / 2 / 3 / 4 KV tiles", ws=False, splits=1,
                   SLM_ATTN_TILE_KV2=_kv2))
for _s in (2, 3):
    for _win in (-1, 63):
        # plan_attn: max_kv_len >= 4 max_q_len and SLM_ATTN_TILE_SPLITS => every kernel of the call writes partials;
        # 131 tokens (one head group per token) keep the token kernel's own wish at 2 shares, so the knob decides
        TILE.append(_c(f"tile_splits{_s}_w{_win}", [65, 40, 5, 1, 17, 2, 1], [300, 200, 65, 200, 129, 2, 0], 16, 8, 128, 16,
                       f"tile kernel split-KV, {_s} shares", window=_win, ws=True, splits=_s, SLM_ATTN_TILE_SPLITS=_s))
_L32 = [(0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129)[i % 11] for i in range(32)]
for _d in (64, 128):
    for _g in (8, 16, 32):
        # decode_on_tile: G >= 8, batch x KV heads = 64 pairs, no forced split
        TILE.append(_c(f"dec_tile_d{_d}_g{_g}", 1, _L32, 2 * _g, 2, _d, 16, "decode on the tile kernel", ws=False, splits=1))
        TILE.append(_c(f"dec_token_d{_d}_g{_g}", 1, _L32, 2 * _g, 2, _d, 16, "the same on the token kernel (GC 8)",
                       SLM_ATTN_TILE_DECODE=0))
TILE.append(_c("mixed", [1, 5, 65, 1, 0, 1], [129, 64, 65, 0, 33, 1], 8, 2, 128, 16,
               "decode + verify + prefill in one call: all three row classes", pad_rows=2))

# MLA: mla_nq = 2 once max_q_len * heads > 32; rows past heads in the last 32-row block are partial tiles; num_splits
# 0 is mla_auto_splits (1 here: max_kv_len < 256)
MLA = []
_blocks, _splits = (1, 16, 64), (1, 2, 3, 8, 0)
for _i, (_d, _h) in enumerate((d, h) for d in (128, 256, 512) for h in (1, 8, 24, 128)):
    _kv = [33, 31] if _h == 1 else [65, 33]
    MLA.append(_c(f"mla_d{_d}_h{_h}", [3, 1], _kv, _h, 1, _d, _blocks[_i % 3],
                  f"mla_kernel<{_d}, NQ {2 if 3 * _h > 32 else 1}>, splits {_splits[_i % 5]}", kind="mla",
                  num_splits=_splits[_i % 5], ws=_splits[_i % 5] > 1))
MLA += [
    _c("mla_decode_b5", 1, [129, 0, 33, 1, 200], 16, 1, 512, 16, "pure decode, batch 5, NQ 1", kind="mla", pad_rows=2),
    _c("mla_decode_b5_s3", 1, [129, 1, 0, 64, 200], 16, 1, 512, 64, "pure decode, batch 5, 3 splits (empty shares)",
       kind="mla", num_splits=3, ws=True),
    _c("mla_prefill", [40, 33], [40, 129], 8, 1, 512, 16, "chunked prefill, NQ 2, several row tiles", kind="mla"),
    _c("mla_prefill_s2", [40, 0, 33], [40, 31, 129], 8, 1, 256, 1,
       "chunked prefill, 2 splits, a sequence without queries", kind="mla", num_splits=2,
       ws=True),
    _c("mla_strided", [1, 6], [65, 129], 16, 1, 512, 16, "q / q_rope are slices of one [T, H, 576] tensor", kind="mla",
       strided=True),
]

ALL = STREAM + TILE + MLA
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)

# worst distance in ulps of T seen on an MI355X (gfx950) over every case, dtype, round and row: no path needed the
# 1-ulp allowance that a path which provably cannot be exact may be given for the spike family
MEASURED = {"spike": 0, "count": 0}
