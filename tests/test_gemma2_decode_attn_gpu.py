"""kernels.paged_decode_attention: decode attention in the model configurations' vocabulary (logit_softcap, a
sliding_window that counts the query's own key, sm_scale defaulting to head_dim ** -0.5) over the paged decode
kernels, against a torch-fp32 reference written here that caps, then masks explicitly, then takes a dense softmax.

Gemma-2's layouts: 8 query heads on 4 KV heads, head_dim 256 (2B / 9B) and 128 with sm_scale 144 ** -0.5 (27B), bf16
and f16.  Tolerances are tests/test_attention_gpu.py's for the same dtypes (its _tol and REL_L2); the reference sees
the inputs as the kernel does, rounded to the test dtype.  Every comparison that is meant to see an option is run
on the CPU reference first with the option off: the two references must differ by MORE than the tolerance."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, HKV, BLOCK = 8, 4, 16
DTYPES = [torch.bfloat16, torch.float16]
ATOL = {torch.bfloat16: (1e-2, 1e-2), torch.float16: (1e-3, 1e-3)}      # test_attention_gpu._tol
REL_L2 = {torch.bfloat16: 5e-3, torch.float16: 6e-4}                     # test_attention_gpu.REL_L2
SOFTCAP_LENS = [1, 17, 200]                    # none a multiple of the page
WINDOW, WINDOW_LENS = 64, [1, 63, 64, 65, 200, 1000]   # 200 -> first key 136, 1000 -> 936, 65 -> 1: all inside a page


def _scale(head_dim):
    """None (the entry point's default, head_dim ** -0.5) for head_dim 256, query_pre_attn_scalar 144 for 128"""
    return None if head_dim == 256 else 144.0 ** -0.5


@functools.lru_cache(maxsize=None)
def _case(kv_lens, head_dim, dtype, q_gain, seed):
    """a pure-decode batch over shuffled pages, rounded to dtype: (q, key_cache, value_cache, kv_cu, table, bcu)
    on the CPU.  q_gain scales the queries so that the scaled scores have that standard deviation."""
    g = torch.Generator().manual_seed(seed)
    nblk = [(n + BLOCK - 1) // BLOCK for n in kv_lens]
    ids = torch.randperm(sum(nblk) + 2, generator=g)[:sum(nblk)]
    sm = head_dim ** -0.5 if _scale(head_dim) is None else _scale(head_dim)
    q = torch.randn(len(kv_lens), H, head_dim, generator=g) * (q_gain / (sm * head_dim ** 0.5))
    kc = torch.randn((sum(nblk) + 2) * BLOCK, HKV, head_dim, generator=g)
    vc = torch.randn((sum(nblk) + 2) * BLOCK, HKV, head_dim, generator=g)
    cu = lambda x: torch.tensor([0] + list(np.cumsum(x)), dtype=torch.int32)  # noqa: E731
    return q.to(dtype), kc.to(dtype), vc.to(dtype), cu(kv_lens), (ids * BLOCK).to(torch.int32), cu(nblk)


@functools.lru_cache(maxsize=None)
def _reference(kv_lens, head_dim, dtype, q_gain, seed, cap, window):
    """[batch, H, head_dim] fp32: s = scale q.k; s = cap tanh(s / cap); keys p <= L - 1 - window masked; softmax; P.V"""
    q, kc, vc, _, table, bcu = _case(kv_lens, head_dim, dtype, q_gain, seed)
    sm = head_dim ** -0.5 if _scale(head_dim) is None else _scale(head_dim)
    out = torch.empty(len(kv_lens), H, head_dim)
    for b, n in enumerate(kv_lens):
        pages = table[bcu[b]:bcu[b + 1]].long()
        slots = (pages[:, None] + torch.arange(BLOCK)[None, :]).reshape(-1)[:n]
        k = kc[slots].float().repeat_interleave(H // HKV, dim=1)      # [n, H, D]
        v = vc[slots].float().repeat_interleave(H // HKV, dim=1)
        s = torch.einsum("hd,nhd->hn", q[b].float(), k) * sm
        if cap > 0:
            s = cap * torch.tanh(s / cap)
        if window > 0:
            p = torch.arange(n)
            s = s.masked_fill((p <= n - 1 - window)[None, :], float("-inf"))
        out[b] = torch.einsum("hn,nhd->hd", torch.softmax(s, dim=-1), v)
    return out.numpy()


def _run(case_key, cap=0.0, window=0, num_splits=0):
    """with a window, every cache row outside it (and every slot no sequence owns) is NaN: a kernel that loads the
    pages in front of the window and masks them afterwards returns NaN (0 * NaN in P.V)"""
    from scalellm_amd import kernels
    kv_lens, head_dim = case_key[0], case_key[1]
    q, kc, vc, kv_cu, table, bcu = _case(*case_key)
    if window > 0:
        seen = []
        for b, n in enumerate(kv_lens):
            p = torch.arange(max(0, n - window), n)
            seen.append(table[bcu[b]:bcu[b + 1]].long()[p // BLOCK] + p % BLOCK)
        seen = torch.cat(seen)
        poisoned = []
        for cache in (kc, vc):
            poisoned.append(torch.full_like(cache, float("nan")))
            poisoned[-1][seen] = cache[seen]
        kc, vc = poisoned
    q, kc, vc, kv_cu, table, bcu = (t.to(DEV) for t in (q, kc, vc, kv_cu, table, bcu))
    out = torch.full_like(q, float("nan"))
    kernels.paged_decode_attention(out, q, kc, vc, kv_cu, table, bcu, BLOCK, max(kv_lens), sm_scale=_scale(head_dim),
                                   logit_softcap=cap, sliding_window=window, num_splits=num_splits)
    torch.cuda.synchronize()
    return out.float().cpu().numpy()


def _rel_l2(out, ref):
    return float(np.sqrt(np.sum(np.square(out.astype(np.float64) - ref)) / np.sum(np.square(ref, dtype=np.float64))))


def _within(out, ref, dtype):
    rtol, atol = ATOL[dtype]
    return bool(np.allclose(out, ref, rtol=rtol, atol=atol)) and _rel_l2(out, ref) <= REL_L2[dtype]


def _check(out, ref, dtype, what):
    rtol, atol = ATOL[dtype]
    rel = _rel_l2(out, ref)
    print(f"\n[decode-attn] {what}: max |err| {np.abs(out - ref).max():.3e}, rel L2 {rel:.3e}")
    assert not np.isnan(out).any(), what
    np.testing.assert_allclose(out, ref, rtol=rtol, atol=atol, err_msg=what)
    assert rel <= REL_L2[dtype], f"{what}: relative L2 error {rel:.2e} > {REL_L2[dtype]:.0e}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("head_dim", [256, 128])
@pytest.mark.parametrize("cap", [50.0, 5.0])
def test_soft_capped_decode_matches_the_reference(cap, head_dim, dtype):
    """the scores are drawn with a standard deviation of 1.2 caps, so the tanh saturates for a good part of them:
    ignoring the cap is far outside the tolerance (asserted on the reference)"""
    key = (tuple(SOFTCAP_LENS), head_dim, dtype, 1.2 * cap, 31)
    ref = _reference(*key, cap, 0)
    assert not _within(_reference(*key, 0.0, 0), ref, dtype), "the inputs do not see the cap"
    _check(_run(key, cap=cap), ref, dtype, f"cap {cap} head_dim {head_dim} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("head_dim", [256, 128])
@pytest.mark.parametrize("cap,num_splits", [(0.0, 0), (0.0, 16), (5.0, 0), (5.0, 16)])
def test_sliding_window_decode_matches_the_reference(cap, num_splits, head_dim, dtype):
    """window 64 over histories of 1 ... 1000 keys on 16-key pages: the window starts inside a page for 65, 200 and
    1000.  num_splits 16 cuts every sequence's VISIBLE range (at most 64 keys) into 16 shares of whole row groups (8 or
    16 rows): at least half of the shares are empty, all but one for the 1-key history -- partials with l = 0 and the
    initial running max, which the combine pass must ignore; 0 is the plan's own count for a 1000-key hint.  cap 5:
    window and soft cap together."""
    gain = 1.2 * cap if cap else 1.0
    key = (tuple(WINDOW_LENS), head_dim, dtype, gain, 47)
    ref = _reference(*key, cap, WINDOW)
    no_window = _reference(*key, cap, 0)
    long_rows = [WINDOW_LENS.index(200), WINDOW_LENS.index(1000)]
    assert not _within(no_window[long_rows], ref[long_rows], dtype), "the inputs do not see the window"
    short_rows = [i for i, n in enumerate(WINDOW_LENS) if n <= WINDOW]
    assert np.array_equal(no_window[short_rows], ref[short_rows])
    _check(_run(key, cap=cap, window=WINDOW, num_splits=num_splits), ref, dtype,
           f"window {WINDOW} cap {cap} splits {num_splits} head_dim {head_dim} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_counts_the_query_token_itself(dtype):
    """sliding_window = W sees exactly W keys: one more or one fewer is outside the tolerance on the reference, and
    the kernel sides with W.  W = 1 is the query's own key alone: the output is its value row."""
    key = ((200, 65), 256, dtype, 1.0, 53)
    ref = _reference(*key, 0.0, WINDOW)
    for other in (WINDOW - 1, WINDOW + 1):
        assert not _within(_reference(*key, 0.0, other), ref, dtype), other
    _check(_run(key, window=WINDOW), ref, dtype, f"window {WINDOW} exactly, {dtype}")
    _check(_run(key, window=1), _reference(*key, 0.0, 1), dtype, f"window 1, {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("head_dim", [256, 128])
def test_options_off_is_the_existing_call_bit_for_bit(head_dim, dtype):
    from scalellm_amd import kernels
    kv_lens = tuple(WINDOW_LENS)
    q, kc, vc, kv_cu, table, bcu = (t.to(DEV) for t in _case(kv_lens, head_dim, dtype, 1.0, 59))
    sm = head_dim ** -0.5 if _scale(head_dim) is None else _scale(head_dim)
    q_cu = torch.arange(len(kv_lens) + 1, dtype=torch.int32, device=DEV)
    for splits in (0, 3):
        old = torch.full_like(q, float("nan"))
        kernels.paged_kv_varlen_mha(old, q, kc, vc, q_cu, kv_cu, table, bcu, None, BLOCK, 1, max(kv_lens), sm,
                                    num_splits=splits)
        new = torch.full_like(q, float("nan"))
        kernels.paged_decode_attention(new, q, kc, vc, kv_cu, table, bcu, BLOCK, max(kv_lens),
                                       sm_scale=_scale(head_dim), logit_softcap=0.0, sliding_window=0,
                                       num_splits=splits)
        torch.cuda.synchronize()
        assert not torch.isnan(new.float()).any() and torch.equal(new, old), splits
    _check(new.float().cpu().numpy(), _reference(kv_lens, head_dim, dtype, 1.0, 59, 0.0, 0), dtype, "options off")


def test_arguments_that_are_not_a_decode_call_are_refused():
    from scalellm_amd import kernels
    q, kc, vc, kv_cu, table, bcu = (t.to(DEV) for t in _case((17, 5), 128, torch.bfloat16, 1.0, 61))
    with pytest.raises(kernels.SlmError):      # two query rows, three sequences' lengths
        kernels.paged_decode_attention(torch.empty_like(q), q, kc, vc, torch.cat([kv_cu, kv_cu[-1:]]), table, bcu,
                                       BLOCK, 17)
    with pytest.raises(kernels.SlmError):
        kernels.paged_decode_attention(torch.empty_like(q), q, kc, vc, kv_cu, table, bcu, BLOCK, 17,
                                       logit_softcap=-1.0)
