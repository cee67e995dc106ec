"""Row gathers and scatters over tensors whose rows lie more than 2 GiB and more than 4 GiB from the base pointer:
the embed form of gemma_norm (token ids select table rows; dim 2048), permute_rows (a hand-built row_id_map sends the
tokens to far rows of the permuted tensor; dim 4096) and unpermute_rows (the same kind of map reads them back, two
rows per token with probabilities).  The far tensor is the K-region view of tests/far_arena.py, its six rows one per
zone (the last row of the view among them).  Every result is bit-equal to the same call on a small compact tensor
that holds the same rows, and what the launch must not write still holds the poison afterwards.

The address arithmetic the far zones exercise:
  gemma.hip     table + id * dim, id = min(max((int64_t)token_ids[tok], 0), vocab - 1)
  permute.hip   permuted + (int64_t)row * V (16-byte vectors), row an int32 map entry; row < permuted_rows, an int64
tests/test_far_offsets_cpu.py shows that each of the three 32-bit slips breaks the row equality."""
import numpy as np
import pytest
import torch

from tests import far_arena as F
from tests import glue_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
COMPACT = np.array([5, 0, 7, 2, 6, 3])    # compact rows of the six far rows (of 8; 1 and 4 stay poison)


@pytest.fixture(scope="module")
def arena():
    torch.cuda.reset_peak_memory_stats()
    holder = [F.allocate()]
    yield holder[0]
    holder.clear()
    torch.cuda.empty_cache()
    print(f"FAR-ARENA rows: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _poison(bits, *shape):
    return torch.full(shape, F.POISON_BITS[bits], dtype=torch.int16, device=DEV).view(TDT[bits])


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _far_and_compact(name, bits, arena, dim, rows=None):
    """(far view, compact tensor, far row ids); rows [6, dim]: written to both (through slices)"""
    far, _ = F.case_rows(name)
    F.refill(arena, bits)
    big = F.view(arena, F.K_BASE, TDT[bits], dim)
    small = _poison(bits, 8, dim)
    if rows is not None:
        for i, (f, c) in enumerate(zip(far, COMPACT)):
            big[int(f):int(f) + 1].copy_(rows[i:i + 1])
            small[int(c):int(c) + 1].copy_(rows[i:i + 1])
    return big, small, far


@pytest.mark.parametrize("bits", ref.BITS)
def test_far_embed_norm(bits, arena):
    from scalellm_amd import kernels
    name, dim = "gemma_embed_norm", 2048
    rows = _randn(1, 6, dim).to(TDT[bits]).to(DEV)
    table, small, far = _far_and_compact(name, bits, arena, dim, rows)
    w = (0.25 * _randn(2, dim)).to(TDT[bits]).to(DEV)
    order = [3, 0, 5, 1, 4, 2, 0]                            # every zone, one row twice
    res = []
    for tab, ids in ((table, far), (small, COMPACT)):
        out, resid = (torch.full((len(order), dim), float("nan"), dtype=TDT[bits], device=DEV) for _ in range(2))
        kernels.gemma_embed_norm(out, resid, tab, _i32(np.asarray(ids)[order]), dim ** 0.5, w, 1e-6)
        torch.cuda.synchronize()
        res.append((_bits(out), _bits(resid)))
    assert np.array_equal(res[0][1], res[1][1]), "residual = T(table[id] * scale) differs from the compact table's"
    assert np.array_equal(res[0][0], res[1][0]), "the normed rows differ from the compact table's"
    scaled = ref.f64_to_t_bits(ref.t_bits_to_f64(_bits(rows), bits)[order] * float(torch.tensor(dim ** 0.5).to(TDT[bits])), bits)
    assert np.array_equal(res[0][1], scaled), "residual is not the selected rows times the rounded scale"
    assert F.untouched(arena, F.rows_written(name), bits)


@pytest.mark.parametrize("bits", ref.BITS)
def test_far_permute_rows(bits, arena):
    from scalellm_amd import kernels
    name, dim = "permute_rows", 4096
    permuted, small, far = _far_and_compact(name, bits, arena, dim)
    tokens = _randn(3, 4, dim).to(TDT[bits]).to(DEV)
    # two maps over four tokens: six mapped rows, two entries -1
    pick = np.array([[0, 1, -1, 2], [3, -1, 4, 5]])
    for dst, ids in ((permuted, far), (small, COMPACT)):
        m = np.where(pick >= 0, np.asarray(ids)[np.maximum(pick, 0)], -1)
        kernels.permute_rows(tokens, _i32(m), dst)
    torch.cuda.synchronize()
    assert F.untouched(arena, F.rows_written(name), bits), "permute_rows wrote outside its mapped rows"
    near, tok = _bits(small), _bits(tokens)
    assert (near[[1, 4]] == F.POISON_BITS[bits]).all()
    for mrow in range(2):
        for t in range(4):
            i = pick[mrow, t]
            if i >= 0:
                got = _bits(permuted[int(far[i]):int(far[i]) + 1])[0]
                assert np.array_equal(got, near[COMPACT[i]]) and np.array_equal(got, tok[t]), (bits, "zone", F.ZONES[5 - i])


@pytest.mark.parametrize("bits", ref.BITS)
def test_far_unpermute_rows(bits, arena):
    from scalellm_amd import kernels
    name, dim = "unpermute_rows", 4096
    rows = _randn(4, 6, dim).to(TDT[bits]).to(DEV)
    permuted, small, far = _far_and_compact(name, bits, arena, dim, rows)
    pick = np.array([[5, 1, -1, 2], [3, 0, 4, -1]])          # token 0: the zones on both sides of 2^32, ...
    probs = (_randn(5, 4, 2).abs() + 0.5).to(DEV)
    outs = []
    for src, ids in ((permuted, far), (small, COMPACT)):
        m = np.where(pick >= 0, np.asarray(ids)[np.maximum(pick, 0)], -1)
        outs.append(_bits(kernels.unpermute_rows(src, _i32(m), probs, 4)))
    torch.cuda.synchronize()
    assert np.array_equal(outs[0], outs[1]), "differs from the compact call"
    r, p = ref.t_bits_to_f64(_bits(rows), bits), probs.double().cpu().numpy()
    want = np.zeros((4, dim))
    for mrow in range(2):
        for t in range(4):
            if pick[mrow, t] >= 0:
                want[t] += p[t, mrow] * r[pick[mrow, t]]
    assert ref.t_ulp_distance(outs[0], ref.f64_to_t_bits(want, bits)).max() <= 1     # fp32 fma chain, one rounding
    assert F.untouched(arena, F.rows_written(name), bits)
