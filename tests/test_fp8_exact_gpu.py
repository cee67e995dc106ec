"""The fp8 weight-only linear (include/slm_hip.h section 15, csrc/dense_fp8.hip) against float64, bit for bit where
the arithmetic is exact: every finite e4m3 code through every byte position of a weight load, integer inputs through
every kernel form, the same bits as the dense kernel on T(W8), the scaled fp32 slab of every K slice, guard rows /
columns / strides, the deferred consumers, random data within the GEMM tolerance, and graph replay."""
import numpy as np
import pytest
import torch

from . import fp8_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn


def _dev(x64, bits):
    return ref.rounded(x64, bits).to(DEV)


def _slabs(handle, M, N):
    """the fp32 slabs [splits, M, N] a deferred call left at the start of its buffer"""
    n = handle.splits * M * N
    assert handle.ptr == handle._keep.data_ptr() and handle.numel == M * N
    return handle._keep[:4 * n].view(torch.float32).view(handle.splits, M, N)


def _rand_w8(g, N, K):
    """uniformly random finite e4m3 codes"""
    codes = torch.randint(0, 256, (N, K), device=DEV, generator=g, dtype=torch.int32)
    codes = torch.where((codes & 0x7F) == 0x7F, torch.zeros_like(codes), codes)
    return codes.to(torch.uint8).view(F8)


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("form", ref.FORMS, ids=lambda f: f"rt{f[0]}nw{f[1]}")
def test_every_code_converts_exactly_in_every_byte_position(form, bits):
    """W[n, k] = code (n + k) mod 256 (NaN codes -> 0), A one-hot: C[m, n] = scale * value(W[n, m + 128 c]), by value
    (-0 arrives as +0 through the accumulator).  Every finite code passes through every byte of a 16-B load, both
    lane halves, both halves of a dword and both chunks."""
    from scalellm_amd import kernels
    M = 128
    K = N = 256
    w8 = ref.code_sweep_weight(N, K).to(DEV).view(F8)
    val = ref.e4m3_value(ref.code_sweep_weight(N, K).numpy())            # [n, k], from the format's definition
    assert not np.isnan(val).any()
    dt = ref.torch_dtype(bits)
    rt, nw = form
    for c in (0, 1):
        a = torch.zeros(M, K, dtype=dt, device=DEV)
        a[torch.arange(M), torch.arange(M) + 128 * c] = 1
        for s in (1.0, 0.5):
            scale = torch.full((N,), s, dtype=torch.float32, device=DEV)
            out = torch.full((M, N), float("nan"), dtype=dt, device=DEV)
            with kernels.tuning(**ref.knobs(rt, nw, 1)):
                info = kernels.fp8_linear_plan(a, w8, scale, out)
                assert (info.row_tiles, info.waves, info.split_k) == (rt, nw, 1)
                kernels.fp8_linear(a, w8, scale, out)
            want = s * val[:, 128 * c:128 * c + M].T                         # [m, n]
            got = ref.as64(out)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (f"c {c} scale {s}: {len(bad)} wrong, first (m, n) = {bad[0]}: code "
                                   f"{int(w8.view(torch.uint8)[bad[0][1], bad[0][0] + 128 * c])} gave "
                                   f"{got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


_CASES_BY_FORM = {f: [c for c in ref.EXACT_CASES if (c[3], c[4]) == f] for f in ref.FORMS}


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("form", ref.FORMS, ids=lambda f: f"rt{f[0]}nw{f[1]}")
def test_integer_inputs_are_exact_in_every_form(form, bits):
    """a, W integers in [-4, 4] (exact in e4m3), a power-of-two scale per channel, integer bias: every partial sum is
    exact in fp32 in any order, so the result is ONE rounding of the float64 reference"""
    from scalellm_amd import kernels
    rng = np.random.default_rng(17)
    for M, N, K, rt, nw, split, with_bias in _CASES_BY_FORM[form]:
        a64, w64, b64 = ref.int_inputs(rng, M, K, N, with_bias)
        s64 = rng.choice(ref.SCALE_CHOICES, size=N)
        a, w8 = _dev(a64, bits), ref.to_w8(w64).to(DEV)
        b = _dev(b64, bits) if with_bias else None
        scale = torch.from_numpy(s64.astype(np.float32)).to(DEV)
        c = torch.full((M, N), float("nan"), dtype=a.dtype, device=DEV)
        with kernels.tuning(**ref.knobs(rt, nw, split)):
            info = kernels.fp8_linear_plan(a, w8, scale, c, b)
            assert (info.row_tiles, info.waves, info.split_k) == (rt, nw, split)
            h = kernels.fp8_linear(a, w8, scale, c, b)
        assert not h
        want = ref.rounded(ref.fp8_ref(a64, w64, s64, b64), bits)
        assert torch.equal(c.cpu(), want), (M, N, K, rt, nw, split, with_bias)


@pytest.mark.parametrize("bits", ref.DTYPES)
def test_same_bits_as_the_dense_kernel_on_the_converted_weight(bits):
    """w_scale = NULL, random codes, random A, the same forced (rt, nw, split): slm_fp8_linear(A, W8) is
    slm_linear(A, T(W8)) bit for bit -- the output, every slab of a deferred split, and the SiLU form.  Pins the
    conversion and the accumulation order of the new loop to the dense one's."""
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(29)
    dt = ref.torch_dtype(bits)
    for M, N, K, rt, nw, split in ref.SAME_BITS_CASES:
        a = torch.randn(M, K, device=DEV, generator=g).to(dt)
        w8 = _rand_w8(g, N, K)
        wt = w8.to(dt)
        assert torch.equal(wt.double().cpu(), torch.from_numpy(ref.w8_as64(w8)))   # e4m3 -> T is exact
        with kernels.tuning(**ref.knobs(rt, nw, split)):
            c_d = torch.full((M, N), float("nan"), dtype=dt, device=DEV)
            c_8 = torch.full((M, N), float("nan"), dtype=dt, device=DEV)
            assert kernels.fp8_linear_plan(a, w8, None, c_8).split_k == split
            kernels.linear(a, wt, c_d)
            kernels.fp8_linear(a, w8, None, c_8)
            assert torch.equal(c_d, c_8), (M, N, K, rt, nw, split)
            h = kernels.linear(a, wt, c_d, defer_reduce=True)
            assert int(h) == split
            slabs_d = _slabs(h, M, N).clone()
            h = kernels.fp8_linear(a, w8, None, c_8, defer_reduce=True)
            assert int(h) == split
            assert torch.equal(slabs_d, _slabs(h, M, N)), (M, N, K, rt, nw, split)
    M, N, K, rt, nw, split = ref.SAME_BITS_SILU
    a = (torch.randn(M, K, device=DEV, generator=g) / 64).to(dt)       # |gate|, |up| of a few units
    w8 = _rand_w8(g, N, K)
    bias = torch.randn(N, device=DEV, generator=g).to(dt)
    with kernels.tuning(**ref.knobs(rt, nw, split)):
        c_d = torch.full((M, N // 2), float("nan"), dtype=dt, device=DEV)
        c_8 = torch.full((M, N // 2), float("nan"), dtype=dt, device=DEV)
        info = kernels.fp8_linear_plan(a, w8, None, c_8, bias, silu_mul=True)
        assert (info.row_tiles, info.waves, info.split_k) == (rt, nw, 1)
        kernels.linear(a, w8.to(dt), c_d, bias, silu_mul=True)
        kernels.fp8_linear(a, w8, None, c_8, bias, silu_mul=True)
        assert torch.equal(c_d, c_8) and not torch.isnan(c_8.float()).any()


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M,N,K,rt,nw,split", ref.SAME_BITS_CASES)
def test_every_slab_is_the_scaled_sum_over_exactly_its_slice(M, N, K, rt, nw, split, bits):
    from scalellm_amd import kernels
    rng = np.random.default_rng(M + K)
    a64, w64, b64 = ref.int_inputs(rng, M, K, N, True)
    s64 = rng.choice(ref.SCALE_CHOICES, size=N)
    a, w8, b = _dev(a64, bits), ref.to_w8(w64).to(DEV), _dev(b64, bits)
    scale = torch.from_numpy(s64.astype(np.float32)).to(DEV)
    c = torch.full((M, N), float("nan"), dtype=a.dtype, device=DEV)
    with kernels.tuning(**ref.knobs(rt, nw, split)):
        info = kernels.fp8_linear_plan(a, w8, scale, c, None, defer_reduce=True)
        assert info.split_k == split
        h = kernels.fp8_linear(a, w8, scale, c, None, defer_reduce=True)
        assert int(h) == split
        slabs = _slabs(h, M, N).clone()
        assert torch.isnan(c).all(), "a deferred call must not write c"
        for j in range(split):
            want = torch.from_numpy(ref.fp8_ref(a64, w64, s64, None, info.slice_k_range(j)).astype(np.float32))
            assert torch.equal(slabs[j].cpu(), want), f"slab {j}: k range {info.slice_k_range(j)}"
        # with a bias the flag is ignored: c is written, reduced, with the bias
        assert not kernels.fp8_linear(a, w8, scale, c, b, defer_reduce=True)
        assert torch.equal(c.cpu(), ref.rounded(ref.fp8_ref(a64, w64, s64, b64), bits))


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M,N,K,rt,nw,split,silu", [(33, 96, 672, 2, 2, 1, False), (5, 32, 1312, 1, 1, 3, False),
                                                    (130, 160, 256, 4, 4, 2, False), (33, 192, 672, 2, 4, 1, True)])
def test_guard_rows_columns_and_strides(M, N, K, rt, nw, split, silu, bits):
    """lda > K, ldw > K, ldc > N: NaN in every padding element of A and c's surroundings, the NaN code 0x7F in every
    padding byte of W -- the padding is never read into a sum and nothing outside c[:M, :n_out] is written"""
    from scalellm_amd import kernels
    rng = np.random.default_rng(3 * M + N)
    a64, w64, b64 = ref.int_inputs(rng, M, K, N, True)
    s64 = rng.choice(ref.SCALE_CHOICES, size=N)
    if silu:
        a64 = a64 / 64.0
    dt = ref.torch_dtype(bits)
    n_out = N // 2 if silu else N
    nan = float("nan")
    a_buf = torch.full((M + 2, K + 24), nan, dtype=dt, device=DEV)
    w_buf = torch.full((N + 2, K + 48), 0x7F, dtype=torch.uint8, device=DEV)
    c_buf = torch.full((M + 4, n_out + 16), nan, dtype=dt, device=DEV)
    s_buf = torch.full((N + 8,), nan, dtype=torch.float32, device=DEV)
    a, w, c = a_buf[1:M + 1, 8:K + 8], w_buf[1:N + 1, 16:K + 16], c_buf[2:M + 2, 8:n_out + 8]
    a.copy_(_dev(a64, bits))
    w.copy_(ref.to_w8(w64).view(torch.uint8).to(DEV))
    scale = s_buf[4:N + 4]
    scale.copy_(torch.from_numpy(s64.astype(np.float32)))
    b = _dev(b64, bits)
    assert w.stride(0) > K and w.stride(0) % 16 == 0 and a.stride(0) > K
    with kernels.tuning(**ref.knobs(rt, nw, split)):
        kernels.fp8_linear(a, w, scale, c, b, silu_mul=silu)             # the bytes of the float8 tensor
    y = ref.fp8_ref(a64, w64, s64, b64)
    if silu:
        want = ref.silu_mul_ref(ref.as64(ref.rounded(y, bits)))
        ulp = 2.0 ** (-7 if bits == "bf16" else -10)
        assert (np.abs(ref.as64(c) - want) <= ulp * np.abs(want) + 1e-6).all()
    else:
        assert torch.equal(c.cpu(), ref.rounded(y, bits))
    mask = torch.ones_like(c_buf, dtype=torch.bool)
    mask[2:M + 2, 8:n_out + 8] = False
    assert torch.isnan(c_buf[mask]).all() and not torch.isnan(c).any()


@pytest.mark.parametrize("bits", ref.DTYPES)
def test_deferred_consumers_equal_the_reduced_tensor(bits):
    """rms_norm, RoPE + KV append and the Gemma sandwich norm fed the slabs of a deferred fp8 call give the bits of
    the same consumer fed the reduced c"""
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(11)
    dt = ref.torch_dtype(bits)
    T, K, H, HKV, D = 7, 1024, 4, 2, 32
    N = (H + 2 * HKV) * D                                               # 256
    a = torch.randn(T, K, device=DEV, generator=g).to(dt)
    w8, scale = kernels.quantize_fp8_weight(torch.randn(N, K, device=DEV, generator=g) * 0.05)
    nw_ = (1 + 0.1 * torch.randn(N, device=DEV, generator=g)).to(dt)
    res0 = torch.randn(T, N, device=DEV, generator=g).to(dt)
    with kernels.tuning(SLM_LINEAR_SPLITK=3):
        c = torch.empty(T, N, dtype=dt, device=DEV)
        assert not kernels.fp8_linear(a, w8, scale, c)
        unwritten = torch.full((T, N), float("nan"), dtype=dt, device=DEV)

        out_a, res_a = torch.empty_like(c), res0.clone()
        kernels.rms_norm(out_a, c, nw_, 1e-5, residual=res_a)
        h = kernels.fp8_linear(a, w8, scale, unwritten, defer_reduce=True)
        assert int(h) == 3
        out_b, res_b = torch.empty_like(c), res0.clone()
        kernels.rms_norm(out_b, unwritten, nw_, 1e-5, residual=res_b, partials=h)
        assert torch.equal(out_a, out_b) and torch.equal(res_a, res_b)

        post = (0.1 * torch.randn(N, device=DEV, generator=g)).to(dt)
        out_a, res_a = torch.empty_like(c), res0.clone()
        kernels.gemma_sandwich_norm(out_a, c, post, res_a, nw_, 1e-6)
        h = kernels.fp8_linear(a, w8, scale, unwritten, defer_reduce=True)
        out_b, res_b = torch.empty_like(c), res0.clone()
        kernels.gemma_sandwich_norm(out_b, unwritten, post, res_b, nw_, 1e-6, partials=h)
        assert torch.equal(out_a, out_b) and torch.equal(res_a, res_b)

        from scalellm_amd.layers import HipAttnHandler
        inv_freq = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32, device=DEV) / D))
        cos_sin = HipAttnHandler.build_cos_sin(D, 64, inv_freq)
        pos = torch.arange(3, 3 + T, dtype=torch.int32, device=DEV)
        slots = torch.arange(5, 5 + T, dtype=torch.int32, device=DEV)

        def rope(qkv, partials):
            kc = torch.zeros(32, HKV, D, dtype=dt, device=DEV)
            vc = torch.zeros_like(kc)
            q = qkv[:, :H * D].view(T, H, D)
            k = qkv[:, H * D:(H + HKV) * D].view(T, HKV, D)
            v = qkv[:, (H + HKV) * D:].view(T, HKV, D)
            kernels.apply_rotary_pos_emb(q, k, pos, cos_sin, D, False, value=v, slot_ids=slots, key_cache=kc,
                                         value_cache=vc, partials=partials)
            return qkv, kc, vc
        qkv_a, kc_a, vc_a = rope(c.clone(), None)
        buf = torch.full((T, N), float("nan"), dtype=dt, device=DEV)
        h = kernels.fp8_linear(a, w8, scale, buf, defer_reduce=True)
        qkv_b, kc_b, vc_b = rope(buf, h)
        assert torch.equal(qkv_a, qkv_b) and torch.equal(kc_a, kc_b) and torch.equal(vc_a, vc_b)


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M,K,N", ref.RANDOM_CASES)
def test_random_data_within_the_gemm_tolerance(M, K, N, bits):
    """randn * 0.02 weights quantised per channel, with bias, against float64 over the SAME e4m3 weights (quantisation
    is the checkpoint's error, not the kernel's); the second run is bit-identical"""
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(M + N)
    dt = ref.torch_dtype(bits)
    a = torch.randn(M, K, device=DEV, generator=g).to(dt)
    w8, scale = kernels.quantize_fp8_weight(torch.randn(N, K, device=DEV, generator=g) * 0.02)
    b = torch.randn(N, device=DEV, generator=g).to(dt)
    c, c2 = torch.empty(M, N, dtype=dt, device=DEV), torch.empty(M, N, dtype=dt, device=DEV)
    kernels.fp8_linear(a, w8, scale, c, b)
    kernels.fp8_linear(a, w8, scale, c2, b)
    want = ref.fp8_ref(ref.as64(a), w8, ref.as64(scale), ref.as64(b))
    err = ref.rel_err(ref.as64(c), want)
    print(f"[fp8] {bits} M={M} K={K} N={N}: mean relative error {err:.3e} (bound {ref.GEMM_TOL[bits]:.0e})")
    assert err < ref.GEMM_TOL[bits]
    assert torch.equal(c, c2)


def test_graph_replay_follows_the_input():
    """one split call and one SiLU call captured; the replay after overwriting `a` in place equals eager on the new a"""
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(23)
    dt = torch.bfloat16
    a = torch.randn(8, 2048, device=DEV, generator=g).to(dt)
    w8, scale = kernels.quantize_fp8_weight(torch.randn(256, 2048, device=DEV, generator=g) * 0.05)
    c, cs = torch.empty(8, 256, dtype=dt, device=DEV), torch.empty(8, 128, dtype=dt, device=DEV)
    assert kernels.fp8_linear_plan(a, w8, scale, c).split_k > 1
    kernels.fp8_linear(a, w8, scale, c)                                 # warm-up: sizes the workspace
    kernels.fp8_linear(a, w8, scale, cs, silu_mul=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kernels.fp8_linear(a, w8, scale, c)
        kernels.fp8_linear(a, w8, scale, cs, silu_mul=True)
    a.copy_(torch.randn(8, 2048, device=DEV, generator=g).to(dt))
    graph.replay()
    torch.cuda.synchronize()
    got, got_s = c.clone(), cs.clone()
    kernels.fp8_linear(a, w8, scale, c)
    kernels.fp8_linear(a, w8, scale, cs, silu_mul=True)
    assert torch.equal(got, c) and torch.equal(got_s, cs)
