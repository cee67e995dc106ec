"""The two copies of the dense weight-stream loop (csrc/dense.hip, csrc/moe_gemm.hip) against each other on random
data: with one expert and an identity row list the grouped GEMM (slm_moe_gemm, weights as the MFMA's B operand,
accumulator C) gives the bits of the dense linear (slm_linear, weights as the A operand, accumulator C^T) with one K
slice and no bias.  Both sum the same k in the same order for every output element, so a change of the chunk order,
the step order or the lane halves' k ranges in one copy only shows here; the integer-input tests (exact in any order)
and the tolerance tests cannot see it."""
import numpy as np
import pytest
import torch

from . import dense_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _identity_list(M):
    """sorted = arange(M) padded to a multiple of 32 with n_flat = M, one expert, all blocks in use"""
    n_pad = (M + 31) // 32 * 32
    srt = torch.full((n_pad,), M, dtype=torch.int32, device=DEV)
    srt[:M] = torch.arange(M, dtype=torch.int32, device=DEV)
    eid = torch.zeros(n_pad // 32, dtype=torch.int32, device=DEV)
    return srt, eid, torch.tensor([n_pad], dtype=torch.int32, device=DEV)


def _inputs(M, N, K, bits, seed):
    rng = np.random.default_rng(seed)
    a = ref.rounded(rng.standard_normal((M, K)), bits).to(DEV)
    w = ref.rounded(rng.standard_normal((N, K)), bits).to(DEV)
    return a, w


def _grouped(a, w, n_out, silu):
    from scalellm_amd import kernels
    M = a.size(0)
    c = torch.full((M, n_out), float("nan"), dtype=a.dtype, device=DEV)
    srt, eid, npad = _identity_list(M)
    kernels.moe_grouped_gemm(a, w[None], c, srt, eid, npad, 1, silu_mul=silu)
    return c


def _dense(a, w, n_out, silu, nw):
    from scalellm_amd import kernels
    c = torch.full((a.size(0), n_out), float("nan"), dtype=a.dtype, device=DEV)
    with kernels.tuning(SLM_LINEAR_RT=1, SLM_LINEAR_NW=nw, SLM_LINEAR_SPLITK=1):
        info = kernels.linear_plan(a, w, c, silu_mul=silu)
        assert (info.row_tiles, info.waves, info.split_k) == (1, nw, 1)
        assert not kernels.linear(a, w, c, silu_mul=silu)
    return c


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("K", [96, 672, 1312])     # tail units only; wrap + one tail unit; wrap + a part-filled ring
@pytest.mark.parametrize("M", [1, 33])
def test_grouped_gemm_with_an_identity_list_gives_the_bits_of_the_dense_linear(M, K, bits):
    N = 96
    a, w = _inputs(M, N, K, bits, 1000 * M + K)
    grouped = _grouped(a, w, N, False)
    assert not bool(torch.isnan(grouped).any())
    for nw in (1, 4):
        assert torch.equal(_dense(a, w, N, False, nw), grouped), (M, K, nw)


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M", [1, 33])
def test_the_silu_epilogues_of_both_give_the_same_bits(M, bits):
    N, K = 192, 672
    a, w = _inputs(M, N, K, bits, 7 * M + K)
    a = a / 8                                          # gate values around +-3: the sigmoid is not saturated
    grouped = _grouped(a, w, N // 2, True)
    assert not bool(torch.isnan(grouped).any())
    for nw in (2, 4):                                  # SiLU pairs waves: never below 2
        assert torch.equal(_dense(a, w, N // 2, True, nw), grouped), (M, nw)
