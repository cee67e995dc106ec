"""Gemma-2's small kernels against plain PyTorch in fp32 on the same (rounded) inputs: RMSNorm with the (1 + w)
weight, GeGLU with the tanh approximation, and the final logit soft cap.  Each kernel computes in fp32 and rounds
ONCE to the tensor dtype, so the bound is one unit in the last place of the result (at most 2 ** -7 relative for
bf16's 8-bit significand, 2 ** -10 for f16's 11 bits: half a unit for the rounding itself, the other half for a
result that the kernels' fast exp / reciprocal moved across a rounding boundary), plus 1e-5 absolute for results
next to zero (the gelu's far negative side).  Sizes: rows that are no multiple of anything,
widths of one and of several 8-wide vectors per thread."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
RTOL = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
ATOL = 1e-5


def _close(got, want, dtype, what):
    got, want = got.float().cpu(), want.cpu()
    assert not torch.isnan(got).any(), what
    err = ((got - want).abs() - ATOL).clamp_min(0) / want.abs().clamp_min(1e-30)
    print(f"\n[gemma2-glue] {what}: max relative error beyond {ATOL} absolute: {float(err.max()):.3e}")
    torch.testing.assert_close(got, want, rtol=RTOL[dtype], atol=ATOL, msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,dim", [(1, 256), (7, 2304), (3, 4608)])
def test_rms_norm_with_one_plus_weight(rows, dim, dtype):
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(rows + dim)
    x = (3.0 * torch.randn(rows, dim, device=DEV, generator=g)).to(dtype)
    w = (0.3 * torch.randn(dim, device=DEV, generator=g)).to(dtype)
    out = torch.full_like(x, float("nan"))
    kernels.gemma_rms_norm(out, x, w, 1e-6)
    xf = x.float()
    want = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6) * (1.0 + w.float())
    _close(out, want, dtype, f"rms_norm(1 + w) {rows} x {dim} {dtype}")
    plain = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6) * w.float()
    assert not torch.allclose(plain.cpu(), want.cpu(), rtol=RTOL[dtype], atol=ATOL)   # the + 1 is seen


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,inter", [(1, 512), (5, 9216)])
def test_geglu_with_the_tanh_approximation(rows, inter, dtype):
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(rows + inter)
    gu = (2.0 * torch.randn(rows, 2 * inter, device=DEV, generator=g)).to(dtype)
    out = torch.full((rows, inter), float("nan"), device=DEV, dtype=dtype)
    kernels.gelu_new_with_mul(gu, out=out)
    want = F.gelu(gu[:, :inter].float(), approximate="tanh") * gu[:, inter:].float()
    _close(out, want, dtype, f"geglu {rows} x {inter} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,vocab", [(1, 512), (3, 256000)])
def test_final_logit_soft_cap(rows, vocab, dtype):
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(rows + vocab)
    x = (25.0 * torch.randn(rows, vocab, device=DEV, generator=g)).to(dtype)      # well into the tanh's flat part
    want = 30.0 * torch.tanh(x.float() / 30.0)
    out = kernels.soft_cap(x.clone(), 30.0)
    _close(out, want, dtype, f"soft cap 30, {rows} x {vocab} {dtype}")
    assert float(out.float().abs().max()) <= 30.0 and float(x.float().abs().max()) > 60.0
