"""GPU tests of the vocabulary-row kernels (csrc/sampling.hip, csrc/rejection.hip, csrc/vocab_row.h) on constructed
inputs whose outputs are determined bit for bit: tests/vocab_exact_cases.py builds them and states why,
tests/test_vocab_exact_cpu.py checks the conditions without a GPU.  Every row of every case is checked:

  exact      the kept set and `processed` (bit-equal, the sign of zero included), tokens, top-n ids, accepted
             lengths, masks; padding columns and the guard row of strided buffers stay untouched; inputs are only read
  probs      on single-plateau survivors bit-equal to float32(1) / float32(count) (vocab_exact_cases.PROBS_ULP_BAR)
  tolerance  logprobs, top-n values and multi-level probs against the float64 reference at test_sampling_gpu.py's
             abs 2e-4 / rel 1e-5 -- the only tolerance here
A repeat of each call is bit-identical.  Every kernel call goes through scalellm_amd.kernels."""
import numpy as np
import pytest
import torch

from tests import vocab_exact_cases as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
OUT_POISON = 7.0      # what an output buffer holds before the call: exact in every type, never a result of a case

S_PARAMS = [pytest.param(c, dt, id=f"{c.name}-{dt}") for c in X.SAMPLING for dt in c.dtypes]
R_PARAMS = [pytest.param(c, dt, id=f"{c.name}-{dt}") for c in X.REJECTION for dt in c.dtypes]


def _bits(t):
    """the bit pattern of a tensor, as a numpy integer array"""
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy()


def _want_bits(a32, dtype):
    return _bits(torch.from_numpy(np.ascontiguousarray(a32, dtype=F32)).to(dtype))


def _close(got, want, where):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), where
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), where
    ok = ~inf & ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=X.LP_REL, atol=X.LP_ABS, err_msg=str(where))


def _dev(P):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in P.items() if v is not None}


# ---- sampling --------------------------------------------------------------------------------------------------------
def _padded(n, V, pad, dtype, fill):
    """an [n + 1, V + pad] buffer (one guard row) holding `fill`, and its [n, V] view"""
    buf = torch.full((n + 1, V + pad), fill, dtype=dtype, device=DEV)
    return buf, buf[:n, :V]


def _call_sampling(case, dtype, x_dev):
    from scalellm_amd import kernels
    n, V = len(case.rows), case.V
    dev = _dev(X.call_params(case))
    in_buf, logits = _padded(n, V, case.pad_in, dtype, X.PAD_VALUE)
    logits.copy_(x_dev)
    in_before = in_buf.clone()
    res = dict(in_buf=in_buf, in_before=in_before)
    if case.entry in ("sample", "process"):
        out_buf, processed = _padded(n, V, case.pad_out, dtype, OUT_POISON)
        res.update(out_buf=out_buf, out_before=out_buf.clone())
    if case.entry == "sample":
        outs = dict(processed=processed, logprobs=torch.full((n,), OUT_POISON, device=DEV))
        if case.n_top:
            outs["top_logprobs"] = torch.full((n, case.n_top), OUT_POISON, device=DEV)
            outs["top_tokens"] = torch.full((n, case.n_top), -7, dtype=torch.int32, device=DEV)
        if case.probs:
            outs["probs"] = torch.full((n, V), OUT_POISON, device=DEV)
        res["tokens"] = kernels.sample(logits, **dev, **outs)
        res["tokens_alone"] = kernels.sample(logits, **dev)     # no output wanted: greedy rows skip the filters
        res.update(outs)
    elif case.entry == "process":
        kernels.logits_process(logits, processed=processed, **dev)
        res["processed"] = processed
    else:
        if case.entry == "inplace":
            kernels.logits_process(logits, **dev)
        elif case.entry == "temp":
            kernels.apply_temperature_penalty(logits, dev["temperatures"])
        elif case.entry == "sparse_fp":
            kernels.apply_frequency_presence_penalty(logits, dev["unique_token_ids"], dev["unique_token_counts"],
                                                     dev["unique_token_lens"], dev["frequency_penalties"],
                                                     dev["presence_penalties"])
        else:
            kernels.apply_repetition_penalty(logits, dev["unique_token_ids"], dev["unique_token_lens"],
                                             dev["repetition_penalties"])
        res["processed"] = logits
    torch.cuda.synchronize()
    return res


def _outside_view_untouched(buf, before, n, V, where):
    b, a = _bits(before), _bits(buf)
    assert np.array_equal(a[n:], b[n:]) and np.array_equal(a[:n, V:], b[:n, V:]), where


@pytest.mark.parametrize("case,dt", S_PARAMS)
def test_sampling_cases_are_exact(case, dt):
    dtype = TORCH[dt]
    n, V = len(case.rows), case.V
    x = np.stack([X.row_values(V, row) for row in case.rows])
    x_dev = torch.from_numpy(x).to(dtype).to(DEV)
    got = _call_sampling(case, dtype, x_dev)
    again = _call_sampling(case, dtype, x_dev)
    for name in ("processed", "tokens", "tokens_alone", "logprobs", "top_logprobs", "top_tokens", "probs", "in_buf",
                 "out_buf"):
        if name in got:   # a repeat is bit-identical
            assert np.array_equal(_bits(got[name]), _bits(again[name])), (case.name, name)
    # strided buffers: the padding columns and the guard row hold what they held
    if case.entry in ("sample", "process"):
        assert np.array_equal(_bits(got["in_buf"]), _bits(got["in_before"])), case.name   # the input is only read
        _outside_view_untouched(got["out_buf"], got["out_before"], n, V, case.name)
    else:
        _outside_view_untouched(got["in_buf"], got["in_before"], n, V, case.name)
    proc = _bits(got["processed"])
    host = {k: got[k].cpu().numpy() for k in ("tokens", "tokens_alone", "logprobs", "top_logprobs", "top_tokens")
            if k in got}
    probs = got["probs"].cpu().numpy() if "probs" in got else None
    for r, row in enumerate(case.rows):
        where = (case.name, dt, r, row.tag)
        e = X.expected(case, r)
        # the kept set and every value, bit for bit (-0 stays -0, the filtered are -inf)
        want = _want_bits(X.expected_processed(case, r), dtype)
        bad = np.nonzero(proc[r] != want)[0]
        assert bad.size == 0, (where, "processed differs at ids", bad[:8].tolist(), proc[r][bad[:8]].tolist(),
                               want[bad[:8]].tolist())
        if case.entry != "sample":
            continue
        assert host["tokens"][r] == e["token"], (where, int(host["tokens"][r]), e["token"])
        assert host["tokens_alone"][r] == e["token"], (where, int(host["tokens_alone"][r]), e["token"])
        _close(host["logprobs"][r], e["logprob"], where)
        if case.n_top:
            assert np.array_equal(host["top_tokens"][r], e["top_ids"]), (where, host["top_tokens"][r], e["top_ids"])
            _close(host["top_logprobs"][r], e["top_lp"], where)
        if probs is not None:
            live = e["live"]
            assert not probs[r][~live].any(), where      # exactly zero off the survivors that carry mass
            if X.survivors_one_plateau(case, r):
                want_p = F32(1) / F32(int(live.sum()))
                dist = np.abs(probs[r][live].view(np.int32).astype(np.int64) - int(want_p.view(np.int32)))
                print(f"{case.name} {dt} row {r} {row.tag}: probs ulp distance {int(dist.max())}")
                assert dist.max() <= X.PROBS_ULP_BAR, (where, int(dist.max()))
            else:
                _close(probs[r][live], e["probs"][live], where)


# ---- rejection -------------------------------------------------------------------------------------------------------
def _strided3(n, rows, V, off, row_stride, seq_stride, dtype):
    """a flat buffer of PAD_VALUE and its [n, rows, V] view at element offset `off`"""
    flat = torch.full((off + n * seq_stride + 16,), X.PAD_VALUE, dtype=dtype, device=DEV)
    return flat, flat.as_strided((n, rows, V), (seq_stride, row_stride, 1), off)


def _call_rejection(case, dt):
    from scalellm_amd import kernels
    dtype = TORCH[dt]
    n, k, V = len(case.seqs), case.k, case.V
    rows_t = k + (1 if case.form == "logits" else 0)
    t_off, t_row, t_seq, d_off, d_row, d_seq = X.rejection_layout(case, dt)
    if case.interleaved:      # a [rows, n, V] buffer viewed as [n, rows, V]
        t_flat = torch.full((rows_t, n, V), X.PAD_VALUE, dtype=dtype, device=DEV)
        target = t_flat.permute(1, 0, 2)
    else:
        t_flat, target = _strided3(n, rows_t, V, t_off, t_row, t_seq, dtype)
    d_flat, draft = _strided3(n, k, V, d_off, d_row, d_seq, torch.float32)
    target.copy_(torch.from_numpy(np.stack([q["target"] for q in case.seqs])).to(dtype))
    draft.copy_(torch.from_numpy(np.stack([q["draft"] for q in case.seqs])))
    eb = target.element_size()
    if not case.interleaved:  # the view really is in the class the case names
        assert {16: 0, 8: 8, 0: eb}[case.t_align] == target.data_ptr() % 16, case.name
        assert {16: 0, 8: 8, 0: 4}[case.d_align] == draft.data_ptr() % 16, case.name
    before = (t_flat.clone(), d_flat.clone())
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=DEV)  # noqa: E731
    kw = dict(target_is_probs=case.form == "probs", mask_out_rejected=case.mask,
              do_sample=torch.tensor([q["do_sample"] for q in case.seqs], device=DEV),
              seeds=torch.tensor([q["seed"] for q in case.seqs], dtype=torch.int64, device=DEV),
              positions=i32([q["pos"] for q in case.seqs]),
              accepted_lens=torch.full((n,), -7, dtype=torch.int32, device=DEV))
    if not case.philox:
        kw["uniform"] = torch.from_numpy(np.stack([q["uniform"] for q in case.seqs])).to(DEV)
    if case.lp:
        kw.update(logprobs=torch.full((n, k + 1), OUT_POISON, device=DEV),
                  top_logprobs=torch.full((n, k + 1, case.n_top), OUT_POISON, device=DEV),
                  top_tokens=torch.full((n, k + 1, case.n_top), -7, dtype=torch.int32, device=DEV))
    tok = kernels.rejection_sample(i32(np.stack([q["drafts"] for q in case.seqs])), draft, target,
                                   i32([q["bonus"] for q in case.seqs]), **kw)
    torch.cuda.synchronize()
    assert torch.equal(t_flat, before[0]) and torch.equal(d_flat, before[1]), case.name     # inputs are only read
    out = dict(tokens=tok, accepted_lens=kw["accepted_lens"])
    out.update({name: kw[name] for name in ("logprobs", "top_logprobs", "top_tokens") if name in kw})
    return out


@pytest.mark.parametrize("case,dt", R_PARAMS)
def test_rejection_cases_are_exact(case, dt):
    got, again = _call_rejection(case, dt), _call_rejection(case, dt)
    for name in got:
        assert np.array_equal(_bits(got[name]), _bits(again[name])), (case.name, name)
    host = {name: t.cpu().numpy() for name, t in got.items()}
    for s in range(len(case.seqs)):
        where = (case.name, dt, s)
        e = X.ref_rejection(case, s)
        assert np.array_equal(host["tokens"][s], e["out"]), (where, host["tokens"][s], e["out"], e["accepted"])
        assert host["accepted_lens"][s] == e["accepted_len"], where
        if case.lp:
            assert np.array_equal(host["top_tokens"][s], e["top_ids"]), where
            _close(host["logprobs"][s], e["logprobs"], where)
            _close(host["top_logprobs"][s], e["top_lp"], where)


@pytest.mark.parametrize("dt", X.DTYPES)
@pytest.mark.parametrize("V", X.GREEDY_V)
def test_greedy_ties_go_to_the_lowest_id(V, dt):
    """all-greedy calls (no draft probabilities): argmax ids at 0, V - 1, inside the tail group and on both sides of
    the thread-stride boundaries; an all -inf row gives token 0; the draft is accepted iff it IS the argmax"""
    from scalellm_amd import kernels
    rows = X.greedy_rows(V)
    n = len(rows)
    target = torch.from_numpy(np.stack([np.stack([row, row]) for row, _ in rows])).to(TORCH[dt]).to(DEV)
    want = np.array([w for _, w in rows])
    for masked in (False, True):
        for hit in (True, False):
            drafts = want if hit else (want + 1) % max(V, 2)
            lens = torch.full((n,), -7, dtype=torch.int32, device=DEV)
            tok = kernels.rejection_sample(torch.tensor(drafts, dtype=torch.int32, device=DEV).view(n, 1), None, target,
                                           torch.full((n,), 3, dtype=torch.int32, device=DEV),
                                           mask_out_rejected=masked, accepted_lens=lens)
            torch.cuda.synchronize()
            tok, lens = tok.cpu().numpy(), lens.cpu().numpy()
            assert np.array_equal(tok[:, 0], want), (V, dt, masked, hit, tok[:, 0], want)
            assert np.array_equal(lens, np.full(n, 2 if hit else 1)), (V, dt, masked, hit)
            assert np.array_equal(tok[:, 1], np.full(n, 3 if hit or not masked else -1)), (V, dt, masked, hit)
