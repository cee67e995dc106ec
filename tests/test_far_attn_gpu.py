"""Attention over caches whose rows lie more than 2 GiB and more than 4 GiB from the cache pointer: cases of
tests/attn_exact_cases.py with their blocks moved into the far zones of tests/far_arena.py (FarAttn), through
kernels.paged_kv_varlen_mha (attn.hip, attn_tile.hip) and kernels.mla_paged_kv (mla.hip), on the dispatch path the
case names (check_path(), as in test_attn_exact_gpu.py).  Per case and dtype, every round of the spike family:

  * rows with a visible target equal V[slot(target), kvh] at 0 ulp (spike_expect of the compact case: relocation
    changes slots, not values);
  * the whole `out` is bit-equal to the same launch over the compact caches (decoy and padding rows included).  For
    the cases of FALL_BACK the compact launch runs under SLM_ATTN_TILE_PF = 4, the register-staged form that the
    launcher gives their far caches (below): decoy rows are real softmax sums, and two forms round them differently;
  * afterwards the arena outside the case's blocks still holds the poison: attention writes no cache.

The address arithmetic the far zones exercise (the slot comes from the block table as an int32; byte offsets reach
2^32 + 64 MiB):
  attn.hip        kbase + (uint64_t)(uint32_t)slot * k_sb  (k_sb a uint32_t: the product is 64-bit)
  attn_tile.hip   the same expression in the register-staged forms (SLM_ATTN_TILE_PF 4 / 2 / 0 and the one-wave class).
                  The LDS-DMA forms (default, 5, KV2) hand index = slot, stride = slot stride to the buffer unit in a
                  structured descriptor, and the unit keeps index * stride to 32 bits (MEASURED below), so the launcher
                  takes them only for caches of at most 4 GiB (slm_attn_args::n_slots * slot stride): over the arena's
                  4 GiB + 64 MiB views the cases pfdef_*, pf5_plain, kv2_1, tile_splits2_w-1 and the prefill rows of
                  mixed run the register-staged 64-row form instead -- what this file checks for them is that
                  fall-back (n_slots given, and n_slots = 0 = unknown), not the DMA forms themselves
  mla.hip         kvbase + (uint64_t)(uint32_t)slot * kv_sb, krbase + ... * kr_sb (64-bit strides)
MLA: the latent cache is the K-region view; the RoPE-key cache is the V-region view with the same slot ids and 128-byte
rows, so it crosses 2^31 only at head_dim 128 (256-byte latent rows) and stays below it at head_dim 512.

MEASURED on an MI355X: with the LDS-DMA forms launched over these views, pfdef_plain, pf5_plain, pfdef_d64, kv2_1,
tile_splits2_w-1 and mixed failed the first bar in both dtypes -- a row at 2^32 + x read the (poison) row at x, rows
below 2^32 were right (the 2^31 mark is no limit) -- and every other case passed; with the fall-back all pass.

tests/test_far_offsets_cpu.py shows that a kernel which took any of these offsets modulo 2^32, modulo 2^31 or
through an int32 would fail the first bar on every case."""
import copy

import numpy as np
import pytest
import torch

from tests import attn_exact_cases as X
from tests import far_arena as F
from tests.attn_exact_cases import f64_to_t_bits, t_ulp_distance
from tests.test_attn_exact_gpu import NAN_BITS, _Call, _explain, _ti

pytestmark = pytest.mark.gpu

# cases whose prefill rows take an LDS-DMA form over caches of at most 4 GiB and the register-staged 64-row form here
FALL_BACK = {"pfdef_plain", "pf5_plain", "pfdef_d64", "kv2_1", "tile_splits2_w-1", "mixed"}
PARAMS = [pytest.param(c, bits, id=f"{c.name}-{bits}") for c in F.ATTN_CASES for bits in c.bits]


@pytest.fixture(scope="module")
def arena():
    torch.cuda.reset_peak_memory_stats()
    holder = [F.allocate()]                                  # a failed allocation is an error, not a skip
    yield holder[0]
    holder.clear()
    torch.cuda.empty_cache()
    print(f"FAR-ARENA attention: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


def _far_call(compact, far, arena):
    """`compact` with its caches replaced by views of the arena that hold the case's blocks in the far zones"""
    case, B = compact.case, compact.case.block
    call = copy.copy(compact)
    if case.kind == "mla":
        call.kv = F.view(arena, F.K_BASE, compact.dt, case.head_dim)
        call.kr = F.view(arena, F.V_BASE, compact.dt, X.MLA_ROPE)[:call.kv.size(0)]   # one slot count for both
        pairs = ((call.kv, compact.kv), (call.kr, compact.kr))
    else:
        call.k = F.view(arena, F.K_BASE, compact.dt, case.kv_heads, case.head_dim)
        call.v = F.view(arena, F.V_BASE, compact.dt, case.kv_heads, case.head_dim)
        pairs = ((call.k, compact.k), (call.v, compact.v))
    for dst, src in pairs:
        for c, f in far.moves:
            dst[f:f + B].copy_(src[c:c + B])
    call.lay = far.lay
    call.idx = (compact.idx[0], compact.idx[1], _ti(far.lay.bt), compact.idx[3])
    return call


@pytest.mark.parametrize("case,bits", PARAMS)
def test_far_spike(case, bits, tune, arena):
    from scalellm_amd import kernels
    tune(**dict(case.knobs))
    F.refill(arena, bits)
    far = F.FarAttn(case)
    compact = _Call(case, bits, "spike")
    call = _far_call(compact, far, arena)
    assert F.untouched(arena, far.written(), bits), "the relocation wrote outside the case's blocks"
    call.check_path()
    n = sum(case.q_lens)
    for r, rnd in enumerate(X.rounds(case)):
        q = X.spike_q(case, rnd)
        got = call.run(q)
        if case.name in FALL_BACK:
            with kernels.tuning(SLM_ATTN_TILE_PF=4):
                near = compact.run(q)
        else:
            near = compact.run(q)
        assert (got[n:] == NAN_BITS[bits]).all(), (case.name, r, "padding rows were written")
        want_bits = f64_to_t_bits(X.spike_expect(case, rnd), bits)
        ex = rnd.exact[:n]
        d = t_ulp_distance(got[:n], want_bits[:n]) * ex[:, :, None]
        assert not d.any(), "far cache: " + _explain(case, bits, r, rnd, got[:n], want_bits[:n], d != 0)
        assert np.array_equal(got, near), (case.name, bits, r, rnd.kind, "differs from the launch over the compact caches",
                                           int((got != near).any(axis=-1).sum()), "rows")
    assert F.untouched(arena, far.written(), bits), (case.name, "an attention launch wrote the cache arena")


@pytest.mark.parametrize("bits", X.BITS)
@pytest.mark.parametrize("name", ["pfdef_plain", "kv2_1"])
def test_unknown_slot_count_counts_as_far(name, bits, tune, arena):
    """slm_attn_args::n_slots = 0: the host does not say how far the caches go, so the launcher must not take the
    LDS-DMA forms -- the far rows still arrive."""
    import ctypes as C

    from scalellm_amd import _lib, kernels
    case = X.BY_NAME[name]
    tune(**dict(case.knobs))
    F.refill(arena, bits)
    far = F.FarAttn(case)
    call = _far_call(_Call(case, bits, "spike"), far, arena)
    rnd = X.rounds(case)[0]
    out, a = call.args(X.spike_q(case, rnd))
    args = kernels._attn_args(*a)
    assert args.n_slots == call.k.size(0) and args.n_slots * call.k.stride(0) * 2 > 2 ** 32
    assert _lib.lib().slm_paged_kv_varlen_mha_kv_near(C.byref(args)) == 0
    args.n_slots = 0
    assert _lib.lib().slm_paged_kv_varlen_mha_kv_near(C.byref(args)) == 0
    assert _lib.lib().slm_paged_kv_varlen_mha_workspace_bytes(C.byref(args)) == 0
    kernels.check(_lib.lib().slm_paged_kv_varlen_mha(C.byref(args), kernels._stream()), "slm_paged_kv_varlen_mha")
    torch.cuda.synchronize()
    n = sum(case.q_lens)
    got = out.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    d = t_ulp_distance(got[:n], f64_to_t_bits(X.spike_expect(case, rnd), bits)[:n]) * rnd.exact[:n][:, :, None]
    assert not d.any(), _explain(case, bits, 0, rnd, got[:n], f64_to_t_bits(X.spike_expect(case, rnd), bits)[:n], d != 0)
