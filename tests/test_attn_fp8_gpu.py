"""GPU tests of the fp8 (e4m3) paged KV cache (include/slm_hip.h section 27): the quantising append against its torch
statement bit for bit, the stream attention against a float64 softmax attention over the DEQUANTISED cache (codes x
scale: quantisation error is not in the comparison; tolerance tests/test_attention_gpu.py's _tol), and one case
whose result is known exactly."""
import numpy as np
import pytest
import torch

from scalellm_amd import kernels
from tests import far_arena as F
from tests.test_attention_gpu import _tol

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
SCALES = (0.5, 2.0, 0.0123, 1.0, 0.25, 3.0, 0.7, 1.5)   # per head, all different: a swapped or dropped scale shows
NAN_CODE = 0x7F


# ------------------------------------------------------------------------------------------------ append
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("head_dim", [64, 128, 256])
def test_append_is_the_torch_statement_bit_for_bit(dtype, head_dim):
    g = torch.Generator().manual_seed(head_dim)
    T, H, KVH, n_slots = 7, 4, 3, 40
    ks, vs = torch.tensor(SCALES[:KVH]), torch.tensor(SCALES[1:KVH + 1])
    qkv = (torch.randn(T, (H + 2 * KVH) * head_dim, generator=g) * 3).to(dtype)
    k = qkv[:, H * head_dim:(H + KVH) * head_dim].view(T, KVH, head_dim)       # strided column slices of the row
    v = qkv[:, (H + KVH) * head_dim:].view(T, KVH, head_dim)
    # beyond +-448 s on every head, and exact ties between two codes under the power-of-two scales (1.0625 lies
    # halfway between the codes 1.0 and 1.125, 0.0009765625 = 2^-10 halfway between 0 and the smallest subnormal)
    for x, s in ((k, ks), (v, vs)):
        x[0, :, 0], x[0, :, 1], x[0, :, 2] = 449.0 * s, -1.0e4, 448.0 * s
        x[1, :2, :4] = torch.tensor([1.0625, -1.0625, 0.0009765625, 1.1875]) * s[:2].view(2, 1)
        x[2, :, 5] = -0.0
    slots = torch.randperm(n_slots, generator=g)[:T].int()
    kc = torch.full((n_slots, KVH, head_dim), 0xA5, dtype=torch.uint8, device=DEV)
    vc = kc.clone()
    qkv_d = qkv.to(DEV)
    kd = qkv_d[:, H * head_dim:(H + KVH) * head_dim].view(T, KVH, head_dim)
    vd = qkv_d[:, (H + KVH) * head_dim:].view(T, KVH, head_dim)
    kernels.set_kv_cache_fp8(slots.to(DEV), kd, vd, kc, vc.view(torch.float8_e4m3fn), ks.to(DEV), vs.to(DEV))
    for cache, x, s in ((kc, k, ks), (vc, v, vs)):
        want = torch.full((n_slots, KVH, head_dim), 0xA5, dtype=torch.uint8)   # untouched slots keep the poison byte
        want[slots.long()] = kernels.quantize_fp8_kv(x, s).view(torch.uint8)
        assert torch.equal(cache.cpu(), want)
    kernels.set_kv_cache_fp8(slots[:0].to(DEV), kd[:0], vd[:0], kc, vc, ks.to(DEV), vs.to(DEV))   # T == 0: a no-op


# ------------------------------------------------------------------------------------------------ attention
def _case(seed, dtype, D, H, KVH, block, q_lens, kv_lens, n_pad=0):
    """Random paged case over byte caches: owned slots hold the codes of N(0, 1) values under per-head scales, every
    other slot holds the NaN code."""
    g = torch.Generator().manual_seed(seed)
    nblk = [(n + block - 1) // block for n in kv_lens]
    ids = torch.randperm(sum(nblk) + 3, generator=g)[:sum(nblk)]
    ks, vs = torch.tensor(SCALES[:KVH]), torch.tensor(SCALES[::-1][:KVH])
    n_slots = (sum(nblk) + 3) * block
    kc = torch.full((n_slots, KVH, D), NAN_CODE, dtype=torch.uint8)
    vc = kc.clone()
    bcu, slots = np.concatenate([[0], np.cumsum(nblk)]), []
    for b, n in enumerate(kv_lens):
        j = torch.arange(n)
        slots.append(ids[bcu[b] + j // block] * block + j % block)
        kc[slots[-1]] = kernels.quantize_fp8_kv(torch.randn(n, KVH, D, generator=g), ks).view(torch.uint8)
        vc[slots[-1]] = kernels.quantize_fp8_kv(torch.randn(n, KVH, D, generator=g), vs).view(torch.uint8)
    q = torch.randn(sum(q_lens) + n_pad, H, D, generator=g).to(dtype)
    i32 = lambda x: torch.tensor(np.asarray(x), dtype=torch.int32, device=DEV)  # noqa: E731
    return dict(q=q.to(DEV), kc=kc.to(DEV), vc=vc.to(DEV), kc_host=kc, vc_host=vc, ks=ks.to(DEV), vs=vs.to(DEV),
                slots=slots, block=block,
                q_lens=q_lens, kv_lens=kv_lens, q_cu=i32(np.concatenate([[0], np.cumsum(q_lens)])),
                kv_cu=i32(np.concatenate([[0], np.cumsum(kv_lens)])), bt=i32(ids * block), bcu=i32(bcu))


def _reference(c, sm_scale, cap=0.0, window=-1):
    """float64 softmax attention over codes x scale, the visible range as section 1 defines it"""
    q, G = c["q"].cpu().double(), c["q"].size(1) // c["kc"].size(1)
    kd = kernels.dequantize_fp8_kv(c["kc_host"], c["ks"].cpu(), torch.float64)
    vd = kernels.dequantize_fp8_kv(c["vc_host"], c["vs"].cpu(), torch.float64)
    out, t = torch.zeros(sum(c["q_lens"]), q.size(1), q.size(2), dtype=torch.float64), 0
    for b, (ql, kl) in enumerate(zip(c["q_lens"], c["kv_lens"])):
        k = kd[c["slots"][b]].repeat_interleave(G, 1)                           # [kl, H, D]
        v = vd[c["slots"][b]].repeat_interleave(G, 1)
        for i in range(ql):
            diag = kl - ql + i
            lo, hi = (max(0, diag - window) if window >= 0 else 0), min(diag + 1, kl)
            s = torch.einsum("hd,khd->hk", q[t], k[lo:hi]) * sm_scale
            if cap > 0:
                s = torch.tanh(s / cap) * cap
            out[t] = torch.einsum("hk,khd->hd", torch.softmax(s, -1), v[lo:hi]) if hi > lo else 0.0
            t += 1
    return out


def _run(c, sm_scale, cap=0.0, window=-1, splits=0, out=None):
    out = torch.full_like(c["q"], 77.0) if out is None else out
    kernels.paged_kv_fp8_attention(out, c["q"], c["kc"], c["vc"], c["q_cu"], c["kv_cu"], c["bt"], c["bcu"], None,
                                   c["block"], max(c["q_lens"]), max(c["kv_lens"]), sm_scale, c["ks"], c["vs"], cap,
                                   window, num_splits=splits)
    return out


def _rows_per_trip(D, H, KVH, n_tokens):
    """KV rows one workgroup covers per loop trip in the launch shape the plan chooses for such a call"""
    q = torch.empty(n_tokens, H, D, dtype=torch.bfloat16, device=DEV)
    kc = torch.empty(8, KVH, D, dtype=torch.uint8, device=DEV)
    i32, s = torch.zeros(n_tokens + 1, dtype=torch.int32, device=DEV), torch.ones(KVH, device=DEV)
    p = kernels.paged_kv_fp8_attention_plan(q, q, kc, kc, i32, i32, i32, i32, None, 16, 1, 130, 1.0, s, s, num_splits=1)
    return p.rows_per_iter * p.ring_depth


# (head_dim, heads, kv heads, block, q lengths, kv lengths, forced splits, window, soft cap); two graph-padding rows
# stand behind every batch.  kv 1 with three splits: a sequence shorter than the split count.
CASES = {
    "d128_g4_mixed": (128, 8, 2, 16, [1] * 6, [1, 15, 16, 17, 130, 64], 1, -1, 0.0),
    "d128_g4_splits3": (128, 8, 2, 16, [1] * 6, [1, 15, 16, 17, 130, 64], 3, -1, 0.0),
    "d64_g1_block8": (64, 4, 4, 8, [1] * 4, [17, 130, 16, 1], 0, -1, 0.0),
    "d64_g1_splits3": (64, 4, 4, 8, [1] * 4, [17, 130, 16, 1], 3, -1, 0.0),
    "d256_g8": (256, 8, 1, 16, [1] * 3, [130, 15, 17], 1, -1, 0.0),
    "d256_g8_splits3": (256, 8, 1, 8, [1] * 3, [130, 15, 17], 3, -1, 0.0),
    "one_past_a_trip": (128, 8, 8, 16, [1] * 2, [None, 16], 1, -1, 0.0),
    "verify_and_chunk": (128, 8, 2, 16, [3, 5, 1], [20, 45, 130], 1, -1, 0.0),
    "verify_and_chunk_splits3": (128, 8, 2, 8, [3, 5, 1], [20, 45, 130], 3, -1, 0.0),
    "window7": (128, 8, 2, 16, [1, 3, 1], [130, 17, 5], 0, 7, 0.0),
    "window7_splits3": (64, 2, 2, 8, [1, 3, 1], [130, 17, 5], 3, 7, 0.0),
    "softcap30": (128, 8, 2, 16, [1, 1, 3], [130, 17, 40], 1, -1, 30.0),
    "softcap30_window7_splits3": (256, 4, 2, 16, [1, 1, 3], [130, 17, 40], 3, 7, 30.0),
    # the launch shapes of large batches: 2 and 8 KV heads per wave load (8: one slot's whole 1 KiB row), 8 waves
    "wave_load_2_heads_splits3": (128, 16, 8, 16, [1] * 62, [(17, 130, 5, 40, 16, 33)[i % 6] for i in range(62)], 3, -1, 0.0),
    "wave_load_8_heads": (128, 8, 8, 16, [1] * 254, [(17, 130, 5, 40, 16, 33)[i % 6] for i in range(254)], 1, -1, 0.0),
    "wave_load_8_heads_8_waves": (128, 32, 8, 8, [1] * 254, [(17, 130, 5, 40, 16, 33)[i % 6] for i in range(254)], 1, -1, 0.0),
    "eight_waves_long_split": (128, 8, 2, 16, [1, 1], [1030, 1100], 1, -1, 0.0),
}
# (KV heads per wave load, waves) the plan must choose for a case; every other case: (1, 4).  The third field forces
# the wave count where a test-sized history would not reach it.
SHAPES = {"wave_load_2_heads_splits3": (2, 4, None), "wave_load_8_heads": (8, 4, None),
          "wave_load_8_heads_8_waves": (8, 8, 8), "eight_waves_long_split": (1, 8, None)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_attention_against_float64_over_the_dequantised_cache(name, dtype, tune):
    D, H, KVH, block, q_lens, kv_lens, splits, window, cap = CASES[name]
    if kv_lens[0] is None:
        kv_lens = [2 * _rows_per_trip(D, H, KVH, sum(q_lens) + 2) + 1] + kv_lens[1:]
    c = _case(len(name), dtype, D, H, KVH, block, q_lens, kv_lens, n_pad=2)
    sm = 1.7 * D ** -0.5
    hpw, waves, force_nw = SHAPES.get(name, (1, 4, None))
    tune(SLM_ATTN8_NW=force_nw)
    p = kernels.paged_kv_fp8_attention_plan(c["q"], c["q"], c["kc"], c["vc"], c["q_cu"], c["kv_cu"], c["bt"], c["bcu"],
                                            None, block, max(q_lens), max(kv_lens), sm, c["ks"], c["vs"], cap, window,
                                            splits)
    assert (p.kv_heads_per_wave, p.waves) == (hpw, waves)
    out = _run(c, sm, cap, window, splits)
    ref = _reference(c, sm, cap, window)
    n = sum(q_lens)
    assert torch.equal(out[n:], torch.full_like(out[n:], 77.0)), "graph-padding rows were written"
    rtol, atol = _tol(dtype)
    got = out[:n].cpu().double()
    assert not got.isnan().any(), "a NaN code of an unowned slot reached the output"
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=rtol, atol=atol)
    assert torch.equal(_run(c, sm, cap, window, splits), out), "repeats differ"


@pytest.mark.parametrize("splits", [1, 3])
def test_a_captured_graph_replays_over_changed_lengths(splits):
    D, H, KVH, block = 128, 8, 2, 16
    c = _case(5, torch.bfloat16, D, H, KVH, block, [1] * 4, [130, 64, 17, 33], n_pad=1)
    sm = D ** -0.5
    out = _run(c, sm, splits=splits)                      # warm-up: the workspace exists before the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _run(c, sm, splits=splits, out=out)
    new_lens = [130, 1, 17, 20]                           # shorter histories in the same blocks, the same hints
    c["kv_cu"].copy_(torch.tensor(np.concatenate([[0], np.cumsum(new_lens)]), dtype=torch.int32))
    c["kv_lens"], c["slots"] = new_lens, [s[:n] for s, n in zip(c["slots"], new_lens)]
    eager = _run(c, sm, splits=splits)
    for _ in range(3):
        out.fill_(77.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    rtol, atol = _tol(torch.bfloat16)
    np.testing.assert_allclose(eager[:4].cpu().double().numpy(), _reference(c, sm).numpy(), rtol=rtol, atol=atol)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["block_end", "split_start", "last_visible"])
def test_a_dominating_key_returns_its_value_row_exactly(where, dtype):
    """One key's score exceeds every other by > 1000 in log2 units: every other weight underflows to 0, so the output
    row is T(v_code * v_scale) of that key's V row, 0 ulp -- with three forced splits, through the combine pass."""
    D, H, KVH, block, kv_len, splits = 128, 8, 2, 16, 130, 3
    c = _case(9, dtype, D, H, KVH, block, [1], [kv_len])
    p = kernels.paged_kv_fp8_attention_plan(c["q"], c["q"], c["kc"], c["vc"], c["q_cu"], c["kv_cu"], c["bt"], c["bcu"],
                                            None, block, 1, kv_len, 1.0, c["ks"], c["vs"], num_splits=splits)
    per = -(-(-(-kv_len // splits)) // p.rows_per_iter) * p.rows_per_iter      # a split's rows: whole iterations
    assert p.n_splits == splits and per < kv_len
    pos = {"block_end": block - 1, "split_start": per, "last_visible": kv_len - 1}[where]
    c["q"].fill_(8.0)
    c["kc"][c["slots"][0]] = 0                                                  # every other key: score 0
    c["kc"][c["slots"][0][pos]] = kernels.quantize_fp8_kv(torch.full((KVH, D), 16.0), torch.ones(KVH)).view(torch.uint8).to(DEV)
    out = _run(c, D ** -0.5, splits=splits)
    v_row = c["vc"][c["slots"][0][pos]].view(torch.float8_e4m3fn)               # [KVH, D]
    want = (v_row.float() * c["vs"].view(-1, 1)).to(dtype).repeat_interleave(H // KVH, 0)
    assert torch.equal(out[0], want)                     # 0 ulp (the code -0.0 comes out as +0.0: P.V sums 0 + -0)
    nz = want != 0
    assert torch.equal(out[0].view(torch.int16)[nz], want.view(torch.int16)[nz])


# ------------------------------------------------------------------------------------------------ beyond 4 GiB
@pytest.fixture(scope="module")
def arena():
    holder = [F.allocate()]
    yield holder[0]
    holder.clear()
    torch.cuda.empty_cache()


def _far_views(arena, KVH, D):
    """byte caches [REGION / row bytes, KVH, D] over region K and region V of the arena, refilled with the poison"""
    F.refill(arena, "bf16")
    return [arena[b // 2:(b + F.REGION) // 2].view(torch.uint8).view(-1, KVH, D) for b in (F.K_BASE, F.V_BASE)]


def test_append_reaches_rows_beyond_4_gib(arena):
    """one token per zone of tests/far_arena.py (below / above 2^31 and 2^32 bytes, the view's last row): the six rows
    hold the torch statement's bytes and nothing else of the arena moved -- a 32-bit slot offset lands in poison"""
    KVH, D = 8, 128
    kc, vc = _far_views(arena, KVH, D)
    slots = F.far_rows(6, KVH * D)
    F.check_placement([(b, int(s) * KVH * D, KVH * D) for b in (F.K_BASE, F.V_BASE) for s in slots])
    g = torch.Generator().manual_seed(1)
    k, v = (torch.randn(6, KVH, D, generator=g).bfloat16() for _ in range(2))
    ks, vs = torch.tensor(SCALES[:KVH]), torch.tensor(SCALES[::-1][:KVH])
    kernels.set_kv_cache_fp8(torch.from_numpy(slots.astype(np.int32)).to(DEV), k.to(DEV), v.to(DEV), kc, vc, ks.to(DEV),
                             vs.to(DEV))
    for cache, x, sc in ((kc, k, ks), (vc, v, vs)):
        got = torch.stack([cache[int(s)] for s in slots]).cpu()
        assert torch.equal(got, kernels.quantize_fp8_kv(x, sc).view(torch.uint8))
    written = [((b + int(s) * KVH * D) // 2, (b + (int(s) + 1) * KVH * D) // 2) for b in (F.K_BASE, F.V_BASE) for s in slots]
    assert F.untouched(arena, written, "bf16")


@pytest.mark.parametrize("splits", [1, 3])
def test_attention_reads_blocks_beyond_4_gib(arena, splits):
    """the blocks of a compact case moved into the far zones (two per zone): every 32-bit alias of an owned byte holds
    the arena's poison (the finite codes 0x80 / 0x43, values the case does not hold), so a narrowed address changes
    the result far beyond the tolerance"""
    D, H, KVH, block, q_lens, kv_lens = 128, 32, 8, 16, [1, 1], [130, 40]
    c = _case(21, torch.bfloat16, D, H, KVH, block, q_lens, kv_lens)
    kc, vc = _far_views(arena, KVH, D)
    compact_bt = c["bt"].cpu().tolist()
    off = F.place(len(compact_bt), block * KVH * D)
    F.check_placement([(b, int(o), block * KVH * D) for b in (F.K_BASE, F.V_BASE) for o in off])
    far_bt = off // (KVH * D)
    assert len(F.zones_hit(off, block * KVH * D)) == 6 and far_bt.max() + block <= kc.size(0) < 2 ** 31
    for s0, f0 in zip(compact_bt, far_bt):
        kc[int(f0):int(f0) + block].copy_(c["kc"][s0:s0 + block])
        vc[int(f0):int(f0) + block].copy_(c["vc"][s0:s0 + block])
    far = dict(c, kc=kc, vc=vc, bt=torch.from_numpy(far_bt.astype(np.int32)).to(DEV))
    sm = 1.7 * D ** -0.5
    out = _run(far, sm, splits=splits)
    assert torch.equal(out, _run(c, sm, splits=splits)), "the far blocks give other bits than the compact ones"
    rtol, atol = _tol(torch.bfloat16)
    np.testing.assert_allclose(out.cpu().double().numpy(), _reference(c, sm).numpy(), rtol=rtol, atol=atol)
