"""Host-side half of the scratch-bounds tests (tests/test_scratch_bounds_gpu.py runs the kernels): every case of
tests/scratch_bounds_cases.py reaches the form it is meant to exercise, its reported workspace matches the layout the
kernels carve out of it, a workspace one byte short (or missing) is refused before any launch, every workspace query
the header declares has a case, and the guard checker itself reports what it must."""
import ctypes as C
import os
import re

import pytest
import torch

from scalellm_amd import _lib
from tests import scratch_bounds_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")
SLM_ERR_WORKSPACE = -3
FAKE_WS = 1 << 24           # a 256-aligned fake workspace address: the refusal comes before anything reads it


def _tuning(case):
    from scalellm_amd import kernels
    return kernels.tuning(**case.knobs)


def _attn_plan(c, L):
    if c.kind == "mla":
        a = S.mla_args(c)
        splits = c.num_splits if c.num_splits > 0 else int(L.slm_mla_paged_kv_auto_splits(C.byref(a)))
        return splits, int(L.slm_mla_paged_kv_workspace_bytes(C.byref(a))), None
    a = S.attn_args(c)
    return (int(L.slm_paged_kv_varlen_mha_auto_splits(C.byref(a))), int(L.slm_paged_kv_varlen_mha_workspace_bytes(C.byref(a))),
            int(L.slm_paged_kv_varlen_mha_decode_kernel(C.byref(a))))


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_case_reaches_its_form_and_its_documented_layout(case):
    L = _lib.lib()
    s = case.spec
    with _tuning(case):
        if case.family in ("attn", "mla"):
            c = s["attn"]
            splits, need, dec = _attn_plan(c, L)
            # [n_tokens][n_heads][slots] partial rows of head_dim values, then their (m, l) pairs
            unit = S.attn_n_tokens(c) * c.heads * (c.head_dim + 2) * 4
            bal = dict(c.knobs).get("SLM_ATTN_BAL", 0) == 2
            assert need > 0 and need % unit == 0 and need // unit >= splits, (need, unit, splits)
            if case.family == "mla":
                assert splits > 1 and need // unit == splits
            elif bal:          # the balanced partition keeps more partial slots than the grid has splits
                assert need // unit > splits, (need // unit, splits)
            else:
                assert splits > 1 and need // unit == splits, (need // unit, splits)
                if c.splits is not None:
                    assert splits == c.splits
            if case.family == "attn" and max(c.q_lens) <= 1:
                assert dec == 0, "a token-kernel decode case runs on the tile kernel"
        elif case.family == "w4":
            g = S.w4_args(s)
            info = _lib.W4PlanInfo()
            assert L.slm_w4a16_gemm_plan(C.byref(g), C.byref(info)) == 0
            need = int(L.slm_w4a16_gemm_workspace_bytes(C.byref(g)))
            M, N = s["M"], s["N"]
            K, _ = S.w4_packed_k_group(s)
            assert info.kernel_name == s["kernel"], (info.kernel_name, s["kernel"])
            if s["kernel"] == "XL_SK":
                assert info.split_k == 1 and info.part_bytes == S.XL_SK_SLOTS + S.XL_SK_SYNC
            elif s["split"]:
                assert info.split_k > 1 and info.part_bytes == info.split_k * M * N * 4
            else:
                assert info.split_k == 1 and info.part_bytes == 0
            assert info.aperm_bytes == (S.round256(M * K * 2) if S.w4_has_perm(s) else 0)
            assert need == info.part_bytes + info.aperm_bytes and need > 0
            if s["consumer"] is not None:
                d = int(L.slm_w4a16_gemm_deferred_splits(C.byref(g)))
                assert d == info.split_k >= 2 and d * M * N * 4 <= need
        elif case.family == "linear":
            M, N = s["M"], s["N"]
            plan, query = getattr(L, case.entry + "_plan"), getattr(L, case.entry + "_workspace_bytes")
            info = _lib.LinearPlanInfo()
            g = S.linear_args(s, False)
            assert plan(C.byref(g), C.byref(info)) == 0
            assert info.split_k == s["split"] > 1
            assert int(query(C.byref(g))) == info.workspace_bytes == s["split"] * M * N * 4
            gd = S.linear_args(s, True)
            d = int(getattr(L, case.entry + "_deferred_splits")(C.byref(gd)))
            assert d == s["split"] and 0 < d * M * N * 4 <= int(query(C.byref(gd)))
        elif case.family == "sampling":
            need = int(L.slm_sample_workspace_bytes(C.byref(S.sampling_args(s, case.entry))))
            assert need == S.round256(s["n_rows"] * s["max_unique"] * 4) > 0
        elif case.family == "rejection":
            need = int(L.slm_rejection_sample_workspace_bytes(C.byref(S.rejection_args(s))))
            assert need == S.round256(s["n_seqs"] * (s["k"] + 1) * 16) > 0
        else:
            assert S.workspace_bytes(case) == 0


def _refusal_args(case):
    """(entry, [argument blocks that need a workspace, with the size their query reports])"""
    L = _lib.lib()
    s = case.spec
    if case.family == "attn":
        a = S.attn_args(s["attn"])
        return L.slm_paged_kv_varlen_mha, [(a, L.slm_paged_kv_varlen_mha_workspace_bytes(C.byref(a)))]
    if case.family == "mla":
        a = S.mla_args(s["attn"])
        return L.slm_mla_paged_kv, [(a, L.slm_mla_paged_kv_workspace_bytes(C.byref(a)))]
    if case.family == "w4":
        g = S.w4_args(s)
        return L.slm_w4a16_gemm, [(g, L.slm_w4a16_gemm_workspace_bytes(C.byref(g)))]
    if case.family == "linear":
        q = getattr(L, case.entry + "_workspace_bytes")
        return getattr(L, case.entry), [(g, q(C.byref(g))) for g in (S.linear_args(s, False), S.linear_args(s, True))]
    if case.family == "sampling":
        a = S.sampling_args(s, case.entry)
        return getattr(L, case.entry), [(a, L.slm_sample_workspace_bytes(C.byref(a)))]
    a = S.rejection_args(s)
    return L.slm_rejection_sample, [(a, L.slm_rejection_sample_workspace_bytes(C.byref(a)))]


@pytest.mark.parametrize("case", [c for c in S.CASES if c.family != "router"], ids=lambda c: c.name)
def test_missing_or_short_workspace_is_refused_before_any_launch(case):
    """fake 256-aligned addresses (never dereferenced): the entry answers SLM_ERR_WORKSPACE for NULL and for one byte
    less than its query reports -- the kernels would otherwise write past what the caller allocated"""
    with _tuning(case):
        fn, blocks = _refusal_args(case)
        for a, need in blocks:
            assert need > 0
            a.workspace, a.workspace_bytes = None, 0
            assert fn(C.byref(a), None) == SLM_ERR_WORKSPACE, (case.name, "NULL workspace")
            a.workspace, a.workspace_bytes = FAKE_WS, need - 1
            assert fn(C.byref(a), None) == SLM_ERR_WORKSPACE, (case.name, "workspace one byte short", need)


def test_router_reports_no_workspace():
    case = S.BY_NAME["moe-router"]
    L = _lib.lib()
    need = C.c_size_t(1)
    s = case.spec
    for dt in (_lib.SLM_BF16, _lib.SLM_F16):
        assert L.slm_moe_router_workspace_bytes(s["T"], s["E"], s["H"], dt, C.byref(need)) == 0 and need.value == 0


def test_every_declared_workspace_query_has_a_case():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"SLM_API\s+size_t\s+(slm_\w+_workspace_bytes)\s*\(", src))
    assert declared, "no workspace query found in the header"
    covered = {S.WORKSPACE_QUERY[c.entry] for c in S.CASES}
    assert declared <= covered, f"workspace queries without a case: {sorted(declared - covered)}"
    for c in S.CASES:
        assert c.entry in S.WORKSPACE_QUERY, c.name


@pytest.mark.parametrize("nbytes", [1, 256, 4096 + 3])
def test_guard_checker_reports_a_byte_on_either_side(nbytes):
    def arena(byte=0xA5):
        buf = torch.full((S.PRE_GUARD + nbytes + S.post_guard_bytes(nbytes),), byte, dtype=torch.uint8)
        buf[S.PRE_GUARD:S.PRE_GUARD + nbytes] = 0xFF
        return buf
    assert S.guard_violations(arena(), nbytes, 0xA5) == []
    buf = arena()
    buf[S.PRE_GUARD:S.PRE_GUARD + nbytes] = 0x11        # the region itself is not the checker's business
    assert S.guard_violations(buf, nbytes, 0xA5) == []
    for off in (-1, nbytes, -S.PRE_GUARD, nbytes + S.post_guard_bytes(nbytes) - 1):
        buf = arena()
        buf[S.PRE_GUARD + off] = 0xA4
        assert S.guard_violations(buf, nbytes, 0xA5) == [off], off
    buf = arena()
    buf[S.PRE_GUARD - 1] = buf[S.PRE_GUARD + nbytes] = 0
    assert S.guard_violations(buf, nbytes, 0xA5) == [-1, nbytes]
    assert S.post_guard_bytes(nbytes) >= max(nbytes, S.POST_MIN)
