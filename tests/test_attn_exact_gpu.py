"""Exact structural tests of the attention kernels on the GPU: every case of tests/attn_exact_cases.py through
kernels.paged_kv_varlen_mha (attn.hip, attn_tile.hip) and kernels.mla_paged_kv (mla.hip), on the dispatch path the
case names.  `out` is pre-filled with NaN.  Per case and dtype:

  spike  every round: rows with a visible target equal V[slot(target), kvh] at 0 ulp; decoy rows (the target is one
         step outside the visible range) match the float64 reference at test_attention_gpu.py's _check tolerances;
  count  one launch: every row is c_d / n within 1 ulp;
  both   rows of sequences without keys are exactly zero, padding rows (and the columns next to a strided view) are
         untouched.

tests/test_attn_exact_cpu.py holds the conditions that make these bars follow from the inputs, and the mutants that
show which mistake each bar catches."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import attn_exact_cases as X
from tests.attn_exact_cases import f64_to_t_bits, t_ulp_distance

pytestmark = pytest.mark.gpu
DEV = "cuda"
TORCH = {"bf16": torch.bfloat16, "f16": torch.float16}
# test_attention_gpu.py: _tol and REL_L2
TOL = {"bf16": (1e-2, 1e-2), "f16": (1e-3, 1e-3)}
REL_L2 = {"bf16": 5e-3, "f16": 6e-4}
NAN_BITS = {bits: int(torch.full((1,), float("nan"), dtype=TORCH[bits]).view(torch.int16).item()) & 0xFFFF for bits in X.BITS}

PARAMS = [pytest.param(c, bits, id=f"{c.name}-{bits}") for c in X.ALL for bits in c.bits]


def _ti(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _bits_of(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


class _Call:
    """One case's device tensors; run(q) launches the kernel of the case on a fresh NaN-filled `out`."""

    def __init__(self, case, bits, family):
        self.case, self.bits, self.dt = case, bits, TORCH[bits]
        self.lay = lay = X.layout(case)
        K, V = X.caches(case, family)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(self.dt)  # noqa: E731  (exact: 16-bit values)
        if case.kind == "mla":
            self.kv, self.kr = up(V[:, 0]), up(K[:, 0, case.head_dim:])
        else:
            self.k, self.v = up(K), up(V)
        self.idx = (_ti(lay.q_cu), _ti(lay.kv_cu), _ti(lay.bt), _ti(lay.bcu))
        al = X.alibi_of(case) if family == "spike" else None
        self.alibi = None if al is None else torch.from_numpy(al).to(DEV)
        self.max_q = max(max(case.q_lens), 1)
        self.max_kv = case.max_kv_hint if case.max_kv_hint is not None else max(case.kv_lens)
        self.guard = None

    def _views(self, q_np):
        """(q, out) -- or, strided: q a slice of a fused projection output, out a view with a wider token stride"""
        case = self.case
        q = torch.from_numpy(np.ascontiguousarray(q_np, dtype=np.float32)).to(DEV).to(self.dt)
        T, H, Dk = q.shape
        D = case.head_dim
        if not case.strided:
            return q, torch.full((T, H, D), float("nan"), dtype=self.dt, device=DEV)
        fused = torch.zeros(T, H * Dk + 128, dtype=self.dt, device=DEV)
        qv = fused[:, :H * Dk].view(T, H, Dk)
        qv.copy_(q)
        self.guard = torch.full((T, H * D + 64), float("nan"), dtype=self.dt, device=DEV)
        return qv, self.guard[:, :H * D].view(T, H, D)

    def args(self, q_np):
        case = self.case
        q, out = self._views(q_np)
        sm = X.sm_scale_of(case)
        if case.kind == "mla":
            D = case.head_dim
            qn, qr = (q[..., :D], q[..., D:]) if case.strided else (q[..., :D].contiguous(), q[..., D:].contiguous())
            return out, (out, qn, qr, self.kv, self.kr, *self.idx, case.block, self.max_q, self.max_kv, sm, case.num_splits)
        return out, (out, q, self.k, self.v, *self.idx, self.alibi, case.block, self.max_q, self.max_kv, sm, case.softcap,
                     case.window, case.num_splits)

    def run(self, q_np):
        from scalellm_amd import kernels
        out, a = self.args(q_np)
        if self.case.kind == "mla":
            kernels.mla_paged_kv(*a[:-1], num_splits=a[-1])
        else:
            kernels.paged_kv_varlen_mha(*a[:-1], num_splits=a[-1])
        torch.cuda.synchronize()
        if self.guard is not None:
            edge = _bits_of(self.guard[:, out.shape[1] * out.shape[2]:])
            assert (edge == NAN_BITS[self.bits]).all(), (self.case.name, "wrote past the strided out view")
        return _bits_of(out)

    def check_path(self):
        """the plan's own answers, where they tell two paths apart: partials + combine, and the decode kernel"""
        from scalellm_amd import _lib, kernels
        case = self.case
        Dk = case.head_dim + (X.MLA_ROPE if case.kind == "mla" else 0)
        _, a = self.args(np.zeros((sum(case.q_lens) + case.pad_rows, case.heads, Dk), np.float32))
        L = _lib.lib()
        if case.kind == "mla":
            need = L.slm_mla_paged_kv_workspace_bytes(C.byref(kernels._mla_args(*a)))
        else:
            ma = kernels._attn_args(*a)
            need = L.slm_paged_kv_varlen_mha_workspace_bytes(C.byref(ma))
            # kernels._attn_args passes the slot count: caches within 4 GiB keep the LDS-DMA prefill forms
            near = self.k.size(0) * self.k.stride(0) * 2 <= 2 ** 32
            assert ma.n_slots == self.k.size(0) and L.slm_paged_kv_varlen_mha_kv_near(C.byref(ma)) == int(near), case.name
            if case.splits is not None:
                assert L.slm_paged_kv_varlen_mha_auto_splits(C.byref(ma)) == case.splits, case.name
            if case.name.startswith("dec_"):
                want = 1 if case.name.startswith("dec_tile") else 0
                assert L.slm_paged_kv_varlen_mha_decode_kernel(C.byref(ma)) == want, case.name
        if case.ws is not None:
            assert (need > 0) == case.ws, (case.name, "workspace bytes", need)


def _row_of(case, lay, t):
    b = int(np.searchsorted(lay.q_cu, t, side="right") - 1)
    return b, t - int(lay.q_cu[b])


def _explain(case, bits, r, rnd, got, want_bits, bad):
    """case, round, row (token, head), target key and slot, and whose V row the output is, if anybody's"""
    lay = X.layout(case)
    _, V = X.caches(case, "spike")
    t, h = (int(x) for x in np.argwhere(bad.any(axis=-1))[0])
    b, qi = _row_of(case, lay, t)
    j = int(rnd.target[t, h])
    slot = int(X.slot_of(lay, b, j)) if j >= 0 else None
    vb = f64_to_t_bits(V, bits)
    same = np.argwhere((vb == got[t, h][None, None, :]).all(axis=-1))
    if len(same):
        s, kvh = (int(x) for x in same[0])
        owner = f"key {int(lay.key_of[s])} of sequence {int(lay.owner[s])}" if lay.owner[s] >= 0 else "a slot nobody owns"
        whose = f"the output is V[slot {s}, kv head {kvh}] = {owner}"
    else:
        whose = "the output is nobody's V row: " + str(X.t_bits_to_f64(got[t, h][:8], bits))
    return (f"{case.name} [{case.path}] {bits} round {r} ({rnd.kind}, {rnd.place}): token {t} (sequence {b}, q index {qi} "
            f"of {case.q_lens[b]}, kv_len {case.kv_lens[b]}) head {h}: target key {j} in slot {slot}, "
            f"{int(bad.sum())} elements off in {int(bad.any(axis=-1).sum())} rows, worst "
            f"{int(t_ulp_distance(got, want_bits).max())} ulps; {whose}")


@pytest.mark.parametrize("case,bits", PARAMS)
def test_spike(case, bits, tune):
    tune(**dict(case.knobs))
    call = _Call(case, bits, "spike")
    call.check_path()
    n = sum(case.q_lens)
    worst = 0
    for r, rnd in enumerate(X.rounds(case)):
        q = X.spike_q(case, rnd)
        got = call.run(q)
        assert (got[n:] == NAN_BITS[bits]).all(), (case.name, r, "padding rows were written")
        want_bits = f64_to_t_bits(X.spike_expect(case, rnd), bits)
        ex = rnd.exact[:n]
        assert ex.any() or rnd.kind.startswith("decoy"), (case.name, r, "a round that checks nothing")
        d = t_ulp_distance(got[:n], want_bits[:n]) * ex[:, :, None]
        worst = max(worst, int(d.max(initial=0)))
        assert not d.any(), _explain(case, bits, r, rnd, got[:n], want_bits[:n], d != 0)
        if not ex.all():
            ref, _ = X.run_ref(case, q, "spike")
            o, w = X.t_bits_to_f64(got[:n], bits)[~ex], ref[:n][~ex]
            rtol, atol = TOL[bits]
            assert not np.isnan(o).any(), (case.name, r, rnd.kind, "NaN in a decoy row")
            np.testing.assert_allclose(o, w, rtol=rtol, atol=atol, err_msg=f"{case.name} {bits} round {r} ({rnd.kind})")
            rel = float(np.sqrt(np.sum(np.square(o - w)) / np.sum(np.square(w))))
            assert rel <= REL_L2[bits], (case.name, r, rnd.kind, "relative L2", rel)
    print(f"ATTN-EXACT spike {case.name} {bits} worst {worst} ulp over {len(X.rounds(case))} rounds")


@pytest.mark.parametrize("case,bits", [p for p in PARAMS if X.has_count(p.values[0])])
def test_count(case, bits, tune):
    tune(**dict(case.knobs))
    call = _Call(case, bits, "count")
    n = sum(case.q_lens)
    Dk = case.head_dim + (X.MLA_ROPE if case.kind == "mla" else 0)
    got = call.run(np.zeros((n + case.pad_rows, case.heads, Dk), np.float32))
    assert (got[n:] == NAN_BITS[bits]).all(), (case.name, "padding rows were written")
    want = X.count_expect(case)[:n]
    d = t_ulp_distance(got[:n], f64_to_t_bits(want, bits))
    print(f"ATTN-EXACT count {case.name} {bits} worst {int(d.max(initial=0))} ulp")
    if d.max(initial=0) > 1:
        lay = X.layout(case)
        t, h = (int(x) for x in np.argwhere((d > 1).any(axis=-1))[0])
        b, qi = _row_of(case, lay, t)
        c = X.count_counts(case)[t]
        seen = X.t_bits_to_f64(got[t, h], bits) * c.sum()
        off = np.flatnonzero(np.abs(seen - c) > 0.25)
        raise AssertionError(
            f"{case.name} [{case.path}] {bits}: token {t} (sequence {b}, q index {qi} of {case.q_lens[b]}, kv_len "
            f"{case.kv_lens[b]}) head {h}: {int((d > 1).any(axis=-1).sum())} rows off, worst {int(d.max())} ulps; this "
            f"row sees {int(c.sum())} keys, out * n differs from the counts in residue classes {off[:8].tolist()}: "
            f"{np.round(seen[off[:8]], 2).tolist()} for {c[off[:8]].tolist()}")
    empty = np.array([case.kv_lens[_row_of(case, X.layout(case), t)[0]] == 0 for t in range(n)], bool)
    assert not (got[:n][empty] & 0x7FFF).any(), (case.name, "rows of sequences without keys must be zero")
