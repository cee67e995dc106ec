"""Multi-head latent attention on the GPU (csrc/mla.hip through kernels.mla_paged_kv) against tests/mla_ref.py, fed
the inputs as rounded to the kernel's dtype.

Element-wise tolerance: the reference tests' own (sm80_mla_pagedkv_test.cu:209-213).  Every comparison also
bounds the relative L2 error with test_attention_gpu.py's REL_L2: that budget is output rounding plus P rounded to
the dtype before P.V, and V here is of the same dtype, so it carries over.  `out` is pre-filled with NaN: none may
remain in rows the call owns.  Block ids are random and may collide (the cache is only read), as in the
reference's test."""
import itertools

import numpy as np
import pytest
import torch

from tests.mla_ref import mla_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROPE = 64
REL_L2 = {torch.bfloat16: 5e-3, torch.float16: 6e-4}
BF16, F16 = torch.bfloat16, torch.float16


def _tol(dtype):
    return (1e-2, 1e-2) if dtype == torch.bfloat16 else (1e-3, 1e-3)


def _rel_l2(out, ref):
    den = float(np.sqrt(np.sum(np.square(ref, dtype=np.float64))))
    return float(np.sqrt(np.sum(np.square(out.astype(np.float64) - ref)))) / den if den > 0 else 0.0


def _check(out, ref, dtype, what=""):
    rtol, atol = _tol(dtype)
    assert not np.isnan(out).any(), f"NaN in output {what}"
    np.testing.assert_allclose(out, ref, rtol=rtol, atol=atol, err_msg=what)
    rel = _rel_l2(out, ref)
    assert rel <= REL_L2[dtype], f"{what}: relative L2 error {rel:.2e} > {REL_L2[dtype]:.0e}"


def _ti(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def make_case(seed, q_lens, kv_lens, block_size, n_heads, head_dim, dtype, dist="rand"):
    """Device tensors of one call: random block ids (collisions allowed), `rand` inputs as in the reference's
    paged test or `randn` as in its contiguous test (sharper softmax)."""
    rng = np.random.default_rng(seed)
    q_cu = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    kv_cu = np.concatenate([[0], np.cumsum(kv_lens)]).astype(np.int32)
    n_blocks = [(k + block_size - 1) // block_size for k in kv_lens]
    bcu = np.concatenate([[0], np.cumsum(n_blocks)]).astype(np.int32)
    total_blocks = sum(n_blocks) + 2
    bt = (rng.integers(0, total_blocks, size=sum(n_blocks)) * block_size).astype(np.int32)
    T, S = int(q_cu[-1]), total_blocks * block_size
    g = torch.Generator(device=DEV).manual_seed(seed)
    f = (lambda *s: torch.rand(*s, device=DEV, generator=g)) if dist == "rand" else \
        (lambda *s: torch.randn(*s, device=DEV, generator=g))
    return dict(q=f(T, n_heads, head_dim).to(dtype), q_rope=f(T, n_heads, ROPE).to(dtype),
                kv_cache=f(S, head_dim).to(dtype), k_rope_cache=f(S, ROPE).to(dtype),
                q_cu=q_cu, kv_cu=kv_cu, bt=bt, bcu=bcu, block_size=block_size, dtype=dtype,
                max_q_len=max(q_lens), max_kv_len=max(kv_lens), sm_scale=1.0 / float(np.sqrt(head_dim + ROPE)))


def run(c, num_splits=0, max_kv_len=None, out=None):
    from scalellm_amd import kernels
    if out is None:
        out = torch.full_like(c["q"], float("nan"))
    kernels.mla_paged_kv(out, c["q"], c["q_rope"], c["kv_cache"], c["k_rope_cache"], _ti(c["q_cu"]), _ti(c["kv_cu"]),
                         _ti(c["bt"]), _ti(c["bcu"]), c["block_size"], c["max_q_len"],
                         c["max_kv_len"] if max_kv_len is None else max_kv_len, c["sm_scale"], num_splits=num_splits)
    torch.cuda.synchronize()
    return out


def ref_of(c):
    n = lambda t: t.float().cpu().numpy()  # noqa: E731  (exactly the rounded values the kernel saw)
    return mla_ref(n(c["q"]), n(c["q_rope"]), n(c["kv_cache"]), n(c["k_rope_cache"]), c["q_cu"], c["kv_cu"], c["bt"],
                   c["bcu"], c["block_size"], c["sm_scale"])


def run_and_check(c, what="", **kw):
    out = run(c, **kw)
    _check(out.float().cpu().numpy(), ref_of(c), c["dtype"], what)
    return out


def _random_lens(seed, batch, max_q_len, max_kv_len):
    """q_len in [1, max_q], kv_len in [q_len, max_kv], as the reference's test draws them."""
    rng = np.random.default_rng(seed)
    q_lens = [int(rng.integers(1, max_q_len + 1)) for _ in range(batch)]
    kv_lens = [int(rng.integers(q, max_kv_len + 1)) if q < max_kv_len else q for q in q_lens]
    return q_lens, kv_lens


# ------------------------------------------------------------------ 1. the reference's grid
GRID = list(itertools.product((F16, BF16), (1, 8, 64), (1, 125), (127, 1000), (128, 256, 512)))


@pytest.mark.parametrize("dtype,block_size,max_q_len,max_kv_len,head_dim", GRID)
def test_reference_grid(dtype, block_size, max_q_len, max_kv_len, head_dim):
    seed = block_size * 7 + max_q_len * 3 + max_kv_len + head_dim
    q_lens, kv_lens = _random_lens(seed, 4, max_q_len, max_kv_len)
    dist = "randn" if (block_size + head_dim // 128) % 2 else "rand"
    run_and_check(make_case(seed, q_lens, kv_lens, block_size, 8, head_dim, dtype, dist), f"{q_lens} {kv_lens} {dist}")


@pytest.mark.parametrize("dtype,n_heads,block_size,max_q_len",
                         list(itertools.product((F16, BF16), (1, 128), (8, 64), (1, 125))))
def test_reference_grid_one_and_128_heads(dtype, n_heads, block_size, max_q_len):
    seed = n_heads + block_size + max_q_len
    q_lens, kv_lens = _random_lens(seed, 2, max_q_len, 1000)
    dist = "randn" if block_size == 8 else "rand"
    run_and_check(make_case(seed, q_lens, kv_lens, block_size, n_heads, 512, dtype, dist), f"{q_lens} {kv_lens} {dist}")


# ------------------------------------------------------------------ 2. the smallest shapes that break tile code
SMALL = [
    # (q_lens, kv_lens, n_heads, head_dim)
    ([1], [1], 8, 512),
    ([1], [31], 8, 512), ([1], [32], 8, 512), ([1], [33], 8, 512), ([1], [64], 8, 512), ([1], [65], 8, 512),
    ([5], [31], 8, 512), ([5], [33], 8, 512), ([7], [65], 8, 512),
    ([40], [40], 8, 512),            # q_len == kv_len: the diagonal starts at 0
    ([3], [70], 8, 512),
    ([3], [70], 24, 512),            # 72 rows: a row tile mixes tokens with different causal limits, the second is partial
    ([3, 2], [50, 45], 24, 512),
    ([1] * 5, [100, 1, 33, 64, 257], 16, 512),   # pure decode, batch 5
    ([3], [70], 24, 128), ([1, 40], [65, 40], 8, 128),
    ([3], [70], 24, 256), ([1, 40], [65, 40], 8, 256),
]


@pytest.mark.parametrize("q_lens,kv_lens,n_heads,head_dim", SMALL)
@pytest.mark.parametrize("dist", ("rand", "randn"))
def test_small_shapes(q_lens, kv_lens, n_heads, head_dim, dist):
    c = make_case(sum(kv_lens) + n_heads, q_lens, kv_lens, 16, n_heads, head_dim, BF16, dist)
    run_and_check(c, f"{q_lens} {kv_lens}")


# ------------------------------------------------------------------ 3. split-KV
@pytest.mark.parametrize("q_len,kv_len", [(1, 5), (1, 1000), (1, 4096), (4, 1000)])
def test_split_kv(q_len, kv_len):
    """Forced splits against the reference and against the unsplit result (rtol 1e-2 / atol 2e-3: the bound
    test_attention_gpu.py uses between plans); at kv_len 5 most splits are empty and must merge as no-ops."""
    c = make_case(kv_len + q_len, [q_len], [kv_len], 64, 16, 512, BF16, "randn")
    ref = ref_of(c)
    base = run(c, num_splits=1).float().cpu().numpy()
    _check(base, ref, BF16, "unsplit")
    for s in ((3,) if q_len > 1 else (2, 3, 8)) + (0,):
        out = run(c, num_splits=s).float().cpu().numpy()
        _check(out, ref, BF16, f"splits={s}")
        np.testing.assert_allclose(out, base, rtol=1e-2, atol=2e-3, err_msg=f"splits={s} vs unsplit")


# ------------------------------------------------------------------ 4. bit-identical repeats
@pytest.mark.parametrize("num_splits", (1, 4))
def test_repeats_are_bit_identical(num_splits):
    c = make_case(11, [1, 3, 40], [900, 333, 40], 8, 16, 512, BF16, "randn")
    a, b = run(c, num_splits=num_splits), run(c, num_splits=num_splits)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    _check(a.float().cpu().numpy(), ref_of(c), BF16)


# ------------------------------------------------------------------ 5. strided views
def test_strided_views():
    """q / q_rope are slices of one [T, H, 576] tensor; out is a view with a larger token stride; nothing outside
    the view changes."""
    H = 16
    c = make_case(5, [1, 6], [77, 130], 16, H, 512, BF16, "randn")
    T = c["q"].size(0)
    fused = torch.cat([c["q"], c["q_rope"]], dim=-1).contiguous()
    c["q"], c["q_rope"] = fused[..., :512], fused[..., 512:]
    assert c["q"].stride(1) == 576 and not c["q_rope"].is_contiguous()
    big = torch.full((T, H + 1, 512), float("nan"), dtype=BF16, device=DEV)
    before = big.clone()
    for splits in (1, 3):
        big.copy_(before)
        out = big[:, :H]
        run(c, num_splits=splits, out=out)
        _check(out.float().cpu().numpy(), ref_of(c), BF16, f"splits={splits}")
        assert torch.equal(big[:, H].view(torch.int16), before[:, H].view(torch.int16))


# ------------------------------------------------------------------ 6. graph padding
@pytest.mark.parametrize("num_splits", (1, 2))
def test_graph_padding_rows_are_left_untouched(num_splits):
    batch, H = 4, 16
    c = make_case(3, [1] * batch, [100, 31, 64, 200], 16, H, 512, BF16)
    pad = lambda t: torch.cat([t, torch.ones(3, *t.shape[1:], dtype=t.dtype, device=DEV)])  # noqa: E731
    c["q"], c["q_rope"] = pad(c["q"]), pad(c["q_rope"])
    out = run(c, num_splits=num_splits)
    assert torch.isnan(out[batch:]).all()
    assert torch.equal(out[batch:].view(torch.int16), torch.full_like(out[batch:], float("nan")).view(torch.int16))
    _check(out[:batch].float().cpu().numpy(), ref_of(c)[:batch], BF16)


# ------------------------------------------------------------------ 7. hipGraph capture and replay
def test_graph_capture_and_replay_over_changed_lengths():
    """One captured decode call (batch 4, 16 heads, max_kv_len hint 512) replayed after new lengths, tables and
    cache rows were written in place; one replay has a sequence longer than the hint."""
    from scalellm_amd import kernels
    batch, H, bs = 4, 16, 16
    steps = [[100, 31, 64, 200], [1, 512, 333, 17], [700, 5, 90, 256]]
    cases = [make_case(20 + i, [1] * batch, kv, bs, H, 512, BF16, "randn") for i, kv in enumerate(steps)]
    n_tbl = max(len(c["bt"]) for c in cases)
    n_slots = max(c["kv_cache"].size(0) for c in cases)
    kvc = torch.zeros(n_slots, 512, dtype=BF16, device=DEV)
    krc = torch.zeros(n_slots, ROPE, dtype=BF16, device=DEV)
    q, qr = torch.zeros_like(cases[0]["q"]), torch.zeros_like(cases[0]["q_rope"])
    q_cu, kv_cu, bcu = _ti(cases[0]["q_cu"]), _ti(cases[0]["kv_cu"]), _ti(cases[0]["bcu"])
    bt = torch.zeros(n_tbl, dtype=torch.int32, device=DEV)
    out = torch.full_like(q, float("nan"))

    def load(c):
        kvc[:c["kv_cache"].size(0)].copy_(c["kv_cache"])
        krc[:c["k_rope_cache"].size(0)].copy_(c["k_rope_cache"])
        q.copy_(c["q"])
        qr.copy_(c["q_rope"])
        kv_cu.copy_(_ti(c["kv_cu"]))
        bcu.copy_(_ti(c["bcu"]))
        bt[:len(c["bt"])].copy_(_ti(c["bt"]))
        out.fill_(float("nan"))

    def call():
        kernels.mla_paged_kv(out, q, qr, kvc, krc, q_cu, kv_cu, bt, bcu, bs, 1, 512, cases[0]["sm_scale"])

    load(cases[0])
    call()  # sizes the split-KV workspace before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    for i, c in enumerate(cases):
        load(c)
        graph.replay()
        torch.cuda.synchronize()
        _check(out.float().cpu().numpy(), ref_of(c), BF16, f"replay {i}: kv_lens {steps[i]}")


# ------------------------------------------------------------------ 8. cache append
def test_cache_append_then_attention():
    from scalellm_amd import kernels
    H, bs, n_slots = 16, 16, 512
    g = torch.Generator(device=DEV).manual_seed(9)
    T = 150
    src = torch.randn(T, 640, device=DEV, generator=g).to(BF16)        # strided sources: one row holds both
    kv, k_rope = src[:, :512], src[:, 512:576]
    slots = torch.randperm(n_slots, device=DEV, generator=g)[:T].int()  # shuffled, non-contiguous
    kvc = torch.full((n_slots, 512), 7.0, dtype=BF16, device=DEV)
    krc = torch.full((n_slots, ROPE), -3.0, dtype=BF16, device=DEV)
    kernels.mla_set_kv_cache(slots, kv, k_rope, kvc, krc)
    torch.cuda.synchronize()
    idx = slots.long()
    assert torch.equal(kvc[idx].view(torch.int16), kv.contiguous().view(torch.int16))
    assert torch.equal(krc[idx].view(torch.int16), k_rope.contiguous().view(torch.int16))
    rest = torch.ones(n_slots, dtype=torch.bool, device=DEV)
    rest[idx] = False
    assert (kvc[rest] == 7.0).all() and (krc[rest] == -3.0).all()
    # the appended history as ONE sequence with block size 1 (the block table is the slot list), then attention
    q = torch.randn(4, H, 512, device=DEV, generator=g).to(BF16)
    qr = torch.randn(4, H, ROPE, device=DEV, generator=g).to(BF16)
    c = dict(q=q, q_rope=qr, kv_cache=kvc, k_rope_cache=krc, q_cu=np.array([0, 4], np.int32),
             kv_cu=np.array([0, T], np.int32), bt=slots.cpu().numpy(), bcu=np.array([0, T], np.int32), block_size=1,
             dtype=BF16, max_q_len=4, max_kv_len=T, sm_scale=1.0 / 24.0)
    run_and_check(c, "append -> attention")
    want = mla_ref(q.float().cpu().numpy(), qr.float().cpu().numpy(), kv.float().cpu().numpy(),
                   k_rope.float().cpu().numpy(), c["q_cu"], c["kv_cu"], np.arange(T), c["bcu"], 1, c["sm_scale"])
    _check(run(c).float().cpu().numpy(), want, BF16, "against the appended rows themselves")


def test_cache_append_skips_negative_slot_ids():
    """Padding rows of a graph-padded step carry a negative slot id: nothing is written for them."""
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(4)
    kv = torch.randn(6, 512, device=DEV, generator=g).to(BF16)
    kr = torch.randn(6, ROPE, device=DEV, generator=g).to(BF16)
    slots = torch.tensor([5, -1, 0, 31, -1, 17], dtype=torch.int32, device=DEV)
    kvc = torch.full((32, 512), 7.0, dtype=BF16, device=DEV)
    krc = torch.full((32, ROPE), -3.0, dtype=BF16, device=DEV)
    kernels.mla_set_kv_cache(slots, kv, kr, kvc, krc)
    torch.cuda.synchronize()
    keep = slots >= 0
    idx = slots[keep].long()
    assert torch.equal(kvc[idx], kv[keep]) and torch.equal(krc[idx], kr[keep])
    rest = torch.ones(32, dtype=torch.bool, device=DEV)
    rest[idx] = False
    assert (kvc[rest] == 7.0).all() and (krc[rest] == -3.0).all()


def test_cpu_tensors_fail_loudly():
    from scalellm_amd import kernels
    from scalellm_amd._lib import SlmError
    c = make_case(1, [1], [8], 8, 8, 128, BF16)
    with pytest.raises(SlmError):
        kernels.mla_paged_kv(torch.empty_like(c["q"]).cpu(), c["q"].cpu(), c["q_rope"].cpu(), c["kv_cache"].cpu(),
                             c["k_rope_cache"].cpu(), _ti(c["q_cu"]), _ti(c["kv_cu"]), _ti(c["bt"]), _ti(c["bcu"]),
                             8, 1, 8, 1.0)
    with pytest.raises(SlmError):
        kernels.mla_set_kv_cache(torch.zeros(1, dtype=torch.int32), c["kv_cache"][:1].cpu(), c["k_rope_cache"][:1].cpu(),
                                 c["kv_cache"].cpu(), c["k_rope_cache"].cpu())
