"""CPU tests of the MoE token permutation boundary (include/slm_hip.h section 14) and of the token dispatchers'
host logic: exported symbols, argument validation before any launch, the references on the reference's hand-worked
examples, the all-to-all plan on the reference's table, and the multi-rank simulation."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from scalellm_amd import _lib, kernels, moe
from scalellm_amd._lib import SlmError

from . import permute_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")
INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -5
F16, BF16, F32 = _lib.SLM_F16, _lib.SLM_BF16, _lib.SLM_F32
SYMBOLS = ["slm_permute_index_map", "slm_permute_mask_map", "slm_permute_rows", "slm_unpermute_rows"]
P = 4096   # a host address that stands for every pointer: no call below may reach a kernel


def test_the_four_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"SLM_API\s+[\w\s\*]+?\b(slm_(?:un)?permute\w*)\s*\(", src)))
    assert declared == SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r"\sT\s+(slm_(?:un)?permute\w*)", out)) == set(SYMBOLS)
    L = _lib.lib()
    for n in SYMBOLS:
        assert getattr(L, n).argtypes is not None and getattr(L, n).restype is C.c_int, n


def test_map_validation_precedes_any_launch():
    L = _lib.lib()
    I, M = L.slm_permute_index_map, L.slm_permute_mask_map
    # slm_permute_index_map(topk_ids, n_tokens, topk, n_experts, row_id_map, tokens_per_expert, stream)
    assert I(None, 8, 2, 8, P, None, None) == INVALID
    assert I(P, 8, 2, 8, None, None, None) == INVALID
    assert I(P, -1, 2, 8, P, None, None) == INVALID
    assert I(P, 8, 0, 8, P, None, None) == INVALID
    assert I(P, 8, 2, 0, P, None, None) == INVALID
    assert I(P, 8, 2, 1025, P, None, None) == INVALID                 # the limit of section 10
    assert I(P, 1 << 28, 8, 8, P, None, None) == INVALID              # n_tokens * topk >= 2^31 - 256
    assert I(None, 0, 2, 8, None, None, None) == 0                    # empty batch, nothing to write
    # slm_permute_mask_map(routing_map, n_tokens, n_experts, row_id_map, tokens_per_expert, n_permuted, stream)
    assert M(None, 8, 8, P, None, None, None) == INVALID
    assert M(P, 8, 8, None, None, None, None) == INVALID
    assert M(P, -1, 8, P, None, None, None) == INVALID
    assert M(P, 8, 0, P, None, None, None) == INVALID
    assert M(P, 8, 1025, P, None, None, None) == INVALID
    assert M(P, 1 << 22, 1024, P, None, None, None) == INVALID
    assert M(None, 0, 8, None, None, None, None) == 0


def test_row_validation_precedes_any_launch():
    L = _lib.lib()
    # slm_permute_rows(permuted, tokens, row_id_map, n_tokens, n_maps, dim, permuted_rows, dtype, stream)
    R = lambda **kw: L.slm_permute_rows(*[dict(dict(p=P, t=P, m=P, T=8, n=2, dim=64, rows=16, dt=BF16), **kw)[k]  # noqa: E731
                                          for k in ("p", "t", "m", "T", "n", "dim", "rows", "dt")], None)
    assert R(p=None) == INVALID and R(t=None) == INVALID and R(m=None) == INVALID
    assert R(T=-1) == INVALID and R(n=0) == INVALID and R(n=1025) == INVALID and R(dim=0) == INVALID
    assert R(rows=-1) == INVALID
    assert R(dt=7) == UNSUPPORTED
    assert R(dim=60) == UNSUPPORTED and R(dim=4, dt=F16) == UNSUPPORTED     # dim * sizeof(T) % 16
    assert R(dim=6, dt=F32) == UNSUPPORTED
    assert R(p=P + 8) == ALIGNMENT and R(t=P + 2) == ALIGNMENT and R(m=P + 2) == ALIGNMENT
    assert R(T=0) == 0 and R(T=0, p=None, t=None, m=None) == 0                # empty batch
    assert R(rows=0) == 0                                                       # no row to store: no launch
    # slm_unpermute_rows(out, permuted, row_id_map, probs, probs_dtype, n_tokens, n_maps, dim, permuted_rows, dtype, stream)
    U = lambda **kw: L.slm_unpermute_rows(*[dict(dict(o=P, p=P, m=P, pr=P, pd=F32, T=8, n=2, dim=64, rows=16, dt=BF16),  # noqa: E731
                                                 **kw)[k]
                                            for k in ("o", "p", "m", "pr", "pd", "T", "n", "dim", "rows", "dt")], None)
    assert U(o=None) == INVALID and U(p=None) == INVALID and U(m=None) == INVALID
    assert U(T=-1) == INVALID and U(n=0) == INVALID and U(dim=-8) == INVALID and U(rows=-1) == INVALID
    assert U(dt=7) == UNSUPPORTED and U(dim=12) == UNSUPPORTED
    assert U(pd=F16) == UNSUPPORTED                                   # probs: fp32 or the tokens' dtype
    assert U(pd=BF16, dt=F32) == UNSUPPORTED
    assert U(o=P + 4) == ALIGNMENT and U(p=P + 8) == ALIGNMENT and U(m=P + 1) == ALIGNMENT
    assert U(pr=P + 2) == ALIGNMENT and U(pr=P + 1, pd=BF16) == ALIGNMENT
    assert U(T=0) == 0 and U(T=0, o=None, p=None, m=None, pr=None) == 0


def test_python_wrappers_fail_loudly_on_cpu_tensors():
    x = torch.zeros(4, 16, dtype=torch.bfloat16)
    ids = torch.zeros(4, 2, dtype=torch.int32)
    mask = torch.zeros(4, 8, dtype=torch.bool)
    rmap = torch.zeros(2, 4, dtype=torch.int32)
    probs = torch.zeros(4, 2)
    for call in (lambda: kernels.permute_index_map(ids, 8), lambda: kernels.permute_mask_map(mask),
                 lambda: kernels.permute_rows(x, rmap, torch.zeros(8, 16, dtype=torch.bfloat16)),
                 lambda: kernels.unpermute_rows(torch.zeros(8, 16, dtype=torch.bfloat16), rmap, probs, 4),
                 lambda: kernels.permute_with_index_map(x, ids), lambda: kernels.permute_with_mask_map(x, mask, 2),
                 lambda: kernels.unpermute_with_index_map(torch.zeros(8, 16, dtype=torch.bfloat16), rmap, probs),
                 lambda: kernels.unpermute_with_mask_map(torch.zeros(8, 16, dtype=torch.bfloat16),
                                                         torch.zeros(8, 4, dtype=torch.int32), torch.zeros(4, 8)),
                 lambda: moe.LocalTokenDispatcher(2).dispatch(x, torch.zeros(4, 8), mask),
                 lambda: moe.LocalTokenDispatcher(2, 8).dispatch_topk(x, probs, ids)):
        with pytest.raises(SlmError):
            call()


# ---- hand-worked cases ----------------------------------------------------------------------------------------------
def test_the_references_index_example():
    rows, counts = ref.index_map([[2, 1], [2, 5]], 8)
    assert rows.reshape(-1).tolist() == [1, 2, 0, 3]
    assert counts.tolist() == [0, 1, 2, 0, 0, 1, 0, 0]


def test_the_references_mask_example():
    mask = np.zeros((4, 4), dtype=bool)
    for t, experts in enumerate(([1, 2], [0, 1], [0, 1], [2, 3])):
        mask[t, experts] = True
    rows, counts = ref.mask_map(mask)
    assert rows.tolist() == [[-1, 0, 1, -1], [2, 3, 4, -1], [5, -1, -1, 6], [-1, -1, -1, 7]]
    assert counts.tolist() == [2, 3, 2, 1]


def test_both_forms_agree_on_distinct_ids_and_foreign_ids_take_no_row():
    rng = np.random.default_rng(3)
    ids = ref.distinct_ids(rng, 33, 3, 8)
    ri, ci = ref.index_map(ids, 8)
    rm, cm = ref.mask_map(ref.ids_to_mask(ids, 8))
    assert np.array_equal(ci, cm)
    for t in range(33):
        for j in range(3):
            assert ri[j, t] == rm[ids[t, j], t]
    ids[0, 0], ids[5, 2] = 8, -1
    ri, ci = ref.index_map(ids, 8)
    assert ri[0, 0] == -1 and ri[2, 5] == -1 and ci.sum() == 33 * 3 - 2
    assert sorted(ri[ri >= 0].tolist()) == list(range(33 * 3 - 2))


def test_unpermute_reference_and_ulp():
    x = np.arange(12, dtype=np.float64).reshape(4, 3)
    rows = np.array([[1, -1], [0, 3]], dtype=np.int32)               # [n_maps = 2, T = 2]
    out, mag = ref.unpermute64(x, rows, np.array([[0.5, 2.0], [1.0, 1.0]]))
    assert np.array_equal(out, np.stack([0.5 * x[1] + 2.0 * x[0], x[3]]))
    assert np.array_equal(mag, np.abs(out))
    assert ref.ulp(1.0, "bf16") == 2.0 ** -7 and ref.ulp(1.5, "f16") == 2.0 ** -10 and ref.ulp(4.0, "f32") == 2.0 ** -21
    assert ref.ulp(0.0, "f16") == 2.0 ** -24


# ---- the all-to-all plan ---------------------------------------------------------------------------------------------
def _table_counts():
    return np.stack([ref.index_map(ids, 8)[1] for ids in ref.REF_TABLE_IDS])


def test_plan_on_the_references_table():
    counts = _table_counts()
    assert counts[0].tolist() == [1, 0, 1, 0, 1, 1, 0, 0]
    for rank in range(4):
        plan = moe.alltoall_plan(counts, rank)
        ins, outs, per_expert, order = ref.alltoall_plan(counts, rank)
        assert plan.input_split_sizes == ins and plan.output_split_sizes == outs
        assert plan.tokens_per_local_expert.tolist() == ref.REF_TABLE_PER_LOCAL_EXPERT[rank] == per_expert.tolist()
        received = np.array(ref.REF_TABLE_RECEIVED[rank])
        assert sum(outs) == received.size
        assert received[order].tolist() == ref.REF_TABLE_ROWS[rank]
        moved = np.empty_like(received)
        moved[plan.reorder.numpy()] = received                        # received row i goes to row reorder[i]
        assert moved.tolist() == ref.REF_TABLE_ROWS[rank]
    assert moe.alltoall_plan(counts, 0).input_split_sizes == [1, 1, 2, 0]


def test_plan_needs_no_reorder_with_one_local_expert_or_one_rank():
    counts = np.arange(16).reshape(4, 4)
    assert moe.alltoall_plan(counts, 1).reorder is None              # one expert per rank
    assert moe.alltoall_plan(counts[:1], 0).reorder is None          # one rank
    with pytest.raises(SlmError):
        moe.alltoall_plan(np.zeros((3, 8)), 0)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("E", [8, 64])
@pytest.mark.parametrize("ep", [1, 2, 4, 8])
def test_simulated_round_trip_returns_every_ranks_tokens(ep, E, k):
    rng = np.random.default_rng(100 * ep + E + k)
    n_tok = [int(rng.integers(0 if r else 1, 17)) for r in range(ep)]           # a rank may have no token at all
    tokens = [rng.integers(-8, 9, size=(n, 32)).astype(np.float64) for n in n_tok]
    ids = [ref.distinct_ids(rng, n, k, E) for n in n_tok]
    probs = [np.full((n, k), 1.0 / k) for n in n_tok]                          # 1 / 4 is exact
    rows, per_expert, combined = ref.simulate(ep, E, ids, tokens, probs)
    L = E // ep
    for r in range(ep):
        assert np.array_equal(combined[r], tokens[r])
        # what a rank's experts see: its experts' rows, expert by expert, source ranks in order
        want = [tokens[s][t] for e in range(r * L, (r + 1) * L) for s in range(ep)
                for t in range(n_tok[s]) for j in range(k) if ids[s][t, j] == e]
        assert np.array_equal(rows[r], np.array(want).reshape(-1, 32))
        assert per_expert[r].tolist() == [sum(int((i == e).sum()) for i in ids) for e in range(r * L, (r + 1) * L)]
        # the product's plan moves the rank-major rows to the same place
        plan = moe.alltoall_plan(np.stack([ref.index_map(i, E)[1] for i in ids]), r)
        _, _, _, order = ref.alltoall_plan(np.stack([ref.index_map(i, E)[1] for i in ids]), r)
        if plan.reorder is None:
            assert np.array_equal(order, np.arange(order.size))
        else:
            assert np.array_equal(plan.reorder.numpy()[order], np.arange(order.size))


# ---- dispatcher bookkeeping over a fake process group ----------------------------------------------------------------
class _FakeGroup:
    """rank `rank` of a 4-way group whose all-gather returns the reference table's counts: metadata only"""

    def __init__(self, rank, counts):
        self.rank, self.world_size, self.counts = rank, counts.shape[0], counts
        self.calls = []

    def allgather_into(self, tensor, output):
        assert tensor.tolist() == self.counts[self.rank].tolist()
        self.calls.append("allgather_into")
        output.copy_(torch.from_numpy(self.counts.astype(np.int32)).view(-1))


def test_dispatcher_bookkeeping_through_a_fake_group():
    counts = _table_counts()
    for rank in range(4):
        pg = _FakeGroup(rank, counts)
        d = moe.AlltoAllTokenDispatcher(8, 2, pg)
        assert (d.ep_size, d.ep_rank, d.n_local_experts, d.topk, d.n_experts) == (4, rank, 2, 2, 8)
        plan = d._gather_plan(torch.from_numpy(counts[rank].astype(np.int32)))
        assert pg.calls == ["allgather_into"]
        assert plan.input_split_sizes == counts[rank].reshape(4, 2).sum(1).tolist()
        assert plan.output_split_sizes == counts[:, 2 * rank:2 * rank + 2].sum(1).tolist()
        assert plan.tokens_per_local_expert.tolist() == ref.REF_TABLE_PER_LOCAL_EXPERT[rank]
        with pytest.raises(SlmError):                                 # the tensors themselves never reach a kernel
            d.dispatch_topk(torch.zeros(2, 32, dtype=torch.bfloat16), torch.full((2, 2), 0.5),
                            torch.tensor(ref.REF_TABLE_IDS[rank], dtype=torch.int32))
    with pytest.raises(SlmError):
        moe.AlltoAllTokenDispatcher(9, 2, _FakeGroup(0, counts))     # 9 experts over 4 ranks
    with pytest.raises(SlmError):
        moe.AlltoAllTokenDispatcher(8, 2, _FakeGroup(0, counts)).combine(torch.zeros(1, 32))


def test_expert_holders_load_their_shard():
    sd = {f"experts.{e}.{w}.weight": torch.full((4, 4), float(e), dtype=torch.bfloat16)
          for e in range(8) for w in ("w1", "w2", "w3")}
    ex = moe.MoEDenseExperts(4, 4, 2, torch.bfloat16, "cpu", expert_offset=4)
    ex.load_state_dict(sd)
    ex.repack()
    assert ex.gate_up.shape == (2, 8, 4) and ex.gate_up[0].unique().tolist() == [4.0]
    assert ex.down[1].unique().tolist() == [5.0]
    whole = moe.MoEDenseExperts(4, 4, 8, torch.bfloat16, "cpu")       # the default keeps today's names
    whole.load_state_dict(sd)
    whole.verify_loaded_weights()


def test_process_group_alltoall_takes_split_sizes():
    from scalellm_amd.model_parallel import LocalShardProcessGroup, ProcessGroup
    x, out = torch.arange(6.0).view(3, 2), torch.zeros(3, 2)
    ProcessGroup().alltoall(x, out, [3], [3])                        # world size 1: a copy
    assert torch.equal(out, x)
    out.zero_()
    LocalShardProcessGroup(4).alltoall(x, out, input_split_sizes=[1, 1, 1, 0], output_split_sizes=[3, 0, 0, 0])
    assert torch.equal(out, x)
    out.zero_()
    ProcessGroup().alltoall(x, out)                                  # today's call still works
    assert torch.equal(out, x)
