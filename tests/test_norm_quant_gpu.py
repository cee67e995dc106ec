"""RMSNorm that writes MXFP4 (slm_rms_norm_mxfp4[_splitk], include/slm_hip.h section 24): an exactly known result
that needs no other kernel, and byte equality with rms_norm followed by quantize_mxfp4_act on random data."""
import numpy as np
import pytest
import torch

from . import w4a4_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
dtypes = pytest.mark.parametrize("bits", ref.DTYPES)
EPS = 1e-5


def _guarded(T, cols, pad):
    buf = torch.full((T, cols + pad), 0xFF, dtype=torch.uint8, device=DEV)
    return buf, buf[:, :cols]


@dtypes
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("dim", [32, 96, 2080, 4128, 8224])     # one quad; NV = 1, 2, 4, 8 with a part-filled last round
def test_unit_rows_times_grid_weights_give_known_codes_and_scales(bits, T, dim):
    """|x| = 1 everywhere: mean square 1, T(x * rsqrt(1 + eps)) = +-1 in both types, so y = +-weight.  weight = an e2m1
    grid value * 2^s per block with a 4 or a 6 in every block: scale byte 127 + s, code = (grid index | sign of x)."""
    from scalellm_amd import kernels
    rng, dt = np.random.default_rng(dim + T), ref.torch_dtype(bits)
    nb = dim // 32
    idx = rng.integers(0, 8, size=(nb, 32))
    idx[np.arange(nb), rng.integers(0, 32, size=nb)] = rng.integers(6, 8, size=nb)
    s = rng.integers(-3, 4, size=nb)
    weight = torch.from_numpy(ref.E2M1[idx] * 2.0 ** s[:, None]).reshape(dim).to(dt).to(DEV)
    neg = rng.integers(0, 2, size=(T, dim))
    x = torch.from_numpy(1.0 - 2.0 * neg).to(dt).to(DEV)
    (qbuf, aq), (sbuf, asc) = _guarded(T, dim // 2, 16), _guarded(T, nb, 3)
    kernels.rms_norm_mxfp4(x, weight, EPS, aq=aq, a_scale=asc)
    assert torch.equal(aq.cpu(), ref.pack(idx.reshape(1, dim) | (neg << 3)))
    assert torch.equal(asc.cpu(), torch.from_numpy((127 + s).astype(np.uint8)).expand(T, nb))
    assert (qbuf[:, dim // 2:] == 0xFF).all() and (sbuf[:, nb:] == 0xFF).all()


@dtypes
@pytest.mark.parametrize("with_out", [False, True], ids=["codes", "codes+T"])
@pytest.mark.parametrize("form", ["plain", "residual", "slabs"])
def test_bytes_equal_rms_norm_then_quantize(bits, form, with_out):
    from scalellm_amd import kernels
    g, dt = torch.Generator(device=DEV).manual_seed(7), ref.torch_dtype(bits)
    T, dim = (7, 256) if form == "slabs" else (5, 4128)
    weight = (1 + 0.1 * torch.randn(dim, device=DEV, generator=g)).to(dt)
    x = torch.randn(T, dim, device=DEV, generator=g).to(dt)
    res_a = torch.randn(T, dim, device=DEV, generator=g).to(dt) if form != "plain" else None
    h = None
    with kernels.tuning(SLM_W4A4_SPLITK=3):
        if form == "slabs":    # x is not written: the GEMM's three fp32 slabs stand for it
            a = torch.randn(T, 1024, device=DEV, generator=g).to(dt)
            w, sc = kernels.quantize_mxfp4_weight(torch.randn(dim, 1024, device=DEV, generator=g) * 0.05)
            x.fill_(float("nan"))
            h = kernels.w4a4_linear(a, w, sc, x, defer_reduce=True)
            assert int(h) == 3
        else:
            x[1, ::32] = float("inf")      # a non-finite value in every block of row 1: scale byte 255
            x[2] = 0                       # an all-zero row: scale byte 127, codes 0
            if res_a is not None:
                res_a[2] = 0
        res_b = res_a.clone() if res_a is not None else None
        want_t, got_t = torch.empty_like(x), torch.full_like(x, 3.0)
        kernels.rms_norm(want_t, x, weight, EPS, residual=res_a, partials=h)
        want_q, want_s = kernels.quantize_mxfp4_act(want_t)
        got_q, got_s = kernels.rms_norm_mxfp4(x, weight, EPS, residual=res_b, partials=h, out=got_t if with_out else None)
    assert torch.equal(got_q, want_q) and torch.equal(got_s, want_s)
    assert torch.equal(got_t.view(torch.int16), want_t.view(torch.int16)) if with_out else (got_t == 3.0).all()
    if res_a is not None:
        assert torch.equal(res_a.view(torch.int16), res_b.view(torch.int16))
    if form != "slabs":
        assert (got_s[1] == 255).all() and (got_s[2] == 127).all() and (got_q[2] == 0).all()
