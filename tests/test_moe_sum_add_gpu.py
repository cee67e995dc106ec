"""slm_moe_sum_add (slm_hip.h section 10): the sum over a token's k expert outputs plus one more row, the shared
experts' output, bit-identical to slm_moe_sum over [T, k + 1, dim] with that row as slot k.

dims: 2048 (one full workgroup of 16-byte pieces), 4104 (513 pieces: no multiple of the 8 x 64 values a wave covers,
a ragged second workgroup) and 100 (no multiple of 8: the scalar path)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("dim", (2048, 4104, 100))
@pytest.mark.parametrize("k", (1, 3, 6))
@pytest.mark.parametrize("T", (1, 33))
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16))
def test_sum_add_is_moe_sum_with_one_more_slot(dtype, T, k, dim):
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(1000 * T + 10 * k + dim)
    whole = torch.randn(T, k + 1, dim, device=DEV, dtype=dtype, generator=g)
    whole[0, :, :8] = torch.tensor([1.0, -1.0, 0.5, 256.0, -256.0, 0.0, 3.0, 1e-3], device=DEV, dtype=dtype)
    want = torch.full((T, dim), float("nan"), device=DEV, dtype=dtype)
    kernels.moe_sum(whole, want)
    inp, addend = whole[:, :k].contiguous(), whole[:, k].contiguous()
    got = torch.full((T, dim), float("nan"), device=DEV, dtype=dtype)
    kernels.moe_sum_add(inp, addend, got)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # control: the sum without the addend is something else
    bare = torch.empty_like(got)
    kernels.moe_sum(inp, bare)
    assert not torch.equal(bare, got)
    # out may be the addend; a repeat gives the same bits
    kernels.moe_sum_add(inp, addend, addend)
    torch.cuda.synchronize()
    assert torch.equal(addend.view(torch.int16), want.view(torch.int16))


def test_wrapper_refuses_mismatched_tensors():
    from scalellm_amd import kernels
    inp = torch.zeros(2, 3, 64, device=DEV, dtype=torch.bfloat16)
    out = torch.zeros(2, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(kernels.SlmError):
        kernels.moe_sum_add(inp, torch.zeros(2, 32, device=DEV, dtype=torch.bfloat16), out)
    with pytest.raises(kernels.SlmError):
        kernels.moe_sum_add(inp, out.half(), out)
