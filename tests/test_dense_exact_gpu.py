"""The dense linear kernel (include/slm_hip.h section 13, csrc/dense.hip) against float64, bit for bit where the
arithmetic is exact: integer inputs (tests/dense_ref.py: every partial sum exact in fp32 in any order) through
every kernel form (row tiles x waves x K split), the fp32 slab of every K slice against the sum over exactly that
slice's k range, guard rows / columns, the SiLU epilogue against the unfused pair, the deferred consumers against
the reduced tensor, random data within the GEMM tolerance, and graph replay."""
import numpy as np
import pytest
import torch

from . import dense_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(x64, bits):
    return ref.rounded(x64, bits).to(DEV)


def _slabs(handle, M, N):
    """the fp32 slabs [splits, M, N] a deferred call left at the start of its buffer"""
    n = handle.splits * M * N
    assert handle.ptr == handle._keep.data_ptr() and handle.numel == M * N
    return handle._keep[:4 * n].view(torch.float32).view(handle.splits, M, N)


_CASES_BY_FORM = {f: [c for c in ref.EXACT_CASES if (c[3], c[4]) == f] for f in ref.FORMS}


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("form", ref.FORMS, ids=lambda f: f"rt{f[0]}nw{f[1]}")
def test_integer_inputs_are_exact_in_every_form(form, bits):
    from scalellm_amd import kernels
    rng = np.random.default_rng(17)
    for M, N, K, rt, nw, split, with_bias in _CASES_BY_FORM[form]:
        a64, w64, b64 = ref.int_inputs(rng, M, K, N, with_bias)
        a, w = _dev(a64, bits), _dev(w64, bits)
        b = _dev(b64, bits) if with_bias else None
        c = torch.full((M, N), float("nan"), dtype=a.dtype, device=DEV)
        with kernels.tuning(**ref.knobs(rt, nw, split)):
            info = kernels.linear_plan(a, w, c, b)
            assert (info.row_tiles, info.waves, info.split_k) == (rt, nw, split)
            h = kernels.linear(a, w, c, b)
        assert not h
        want = ref.rounded(ref.linear_ref(a64, w64, b64), bits)
        assert torch.equal(c.cpu(), want), (M, N, K, rt, nw, split, with_bias)


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M,N,K,rt,nw,split", [(33, 96, 1312, 2, 2, 3), (1, 160, 672, 1, 4, 5), (129, 32, 640, 4, 4, 2),
                                               (65, 96, 256, 1, 1, 2), (160, 160, 1312, 2, 4, 5)])
def test_every_slab_is_the_sum_over_exactly_its_slice(M, N, K, rt, nw, split, bits):
    from scalellm_amd import kernels
    rng = np.random.default_rng(M + K)
    a64, w64, b64 = ref.int_inputs(rng, M, K, N, True)
    a, w, b = _dev(a64, bits), _dev(w64, bits), _dev(b64, bits)
    c = torch.full((M, N), float("nan"), dtype=a.dtype, device=DEV)
    with kernels.tuning(**ref.knobs(rt, nw, split)):
        info = kernels.linear_plan(a, w, c, None, defer_reduce=True)
        assert info.split_k == split
        h = kernels.linear(a, w, c, None, defer_reduce=True)
        assert int(h) == split
        slabs = _slabs(h, M, N).clone()
        assert torch.isnan(c).all(), "a deferred call must not write c"
        for j in range(split):
            want = torch.from_numpy(ref.linear_ref(a64, w64, None, info.slice_k_range(j)).astype(np.float32))
            assert torch.equal(slabs[j].cpu(), want), f"slab {j}: k range {info.slice_k_range(j)}"
        assert torch.equal(slabs.sum(0).cpu(), torch.from_numpy(ref.linear_ref(a64, w64).astype(np.float32)))
        # with a bias the flag is ignored: c is written, reduced, with the bias
        assert not kernels.linear(a, w, c, b, defer_reduce=True)
        assert torch.equal(c.cpu(), ref.rounded(ref.linear_ref(a64, w64, b64), bits))
        # the non-deferred split result = T(sum of the deferred slabs in slice order + bias)
        s = torch.zeros(M, N, dtype=torch.float32, device=DEV)
        for j in range(split):
            s += slabs[j]
        assert torch.equal(c, (s + b.float()[None, :]).to(c.dtype))


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M,N,K,rt,nw,split,silu", [(33, 96, 672, 2, 2, 1, False), (5, 32, 1312, 1, 1, 3, False),
                                                    (130, 160, 256, 4, 4, 2, False), (33, 192, 672, 2, 4, 1, True)])
def test_guard_rows_columns_and_strides(M, N, K, rt, nw, split, silu, bits):
    """lda > K, ldw > K, ldc > N with NaN in every padding element and guard rows around c: the padding is never read
    into a sum and nothing outside c[:M, :n_out] is written"""
    from scalellm_amd import kernels
    rng = np.random.default_rng(3 * M + N)
    a64, w64, b64 = ref.int_inputs(rng, M, K, N, True)
    if silu:
        a64 = a64 / 64.0                                           # |gate|, |up| <= 176: the product stays inside f16
    dt = ref.torch_dtype(bits)
    n_out = N // 2 if silu else N
    nan = float("nan")
    a_buf = torch.full((M + 2, K + 24), nan, dtype=dt, device=DEV)
    w_buf = torch.full((N + 2, K + 40), nan, dtype=dt, device=DEV)
    c_buf = torch.full((M + 4, n_out + 16), nan, dtype=dt, device=DEV)
    a, w, c = a_buf[1:M + 1, 8:K + 8], w_buf[1:N + 1, 16:K + 16], c_buf[2:M + 2, 8:n_out + 8]
    a.copy_(_dev(a64, bits))
    w.copy_(_dev(w64, bits))
    b = _dev(b64, bits)
    with kernels.tuning(**ref.knobs(rt, nw, split)):
        kernels.linear(a, w, c, b, silu_mul=silu)
    y = ref.linear_ref(a64, w64, b64)
    if silu:
        # (the exact comparison with the unfused pair is test_silu_epilogue_...; here: one ulp of T around float64)
        want = ref.silu_mul_ref(ref.as64(ref.rounded(y, bits)))
        ulp = 2.0 ** (-7 if bits == "bf16" else -10)
        assert (np.abs(ref.as64(c) - want) <= ulp * np.abs(want) + 1e-6).all()
    else:
        assert torch.equal(c.cpu(), ref.rounded(y, bits))
    mask = torch.ones_like(c_buf, dtype=torch.bool)
    mask[2:M + 2, 8:n_out + 8] = False
    assert torch.isnan(c_buf[mask]).all() and not torch.isnan(c).any()


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("N,K", [(64, 128), (192, 672)])
@pytest.mark.parametrize("with_bias", [False, True])
def test_silu_epilogue_equals_linear_then_silu_and_mul(N, K, with_bias, bits):
    from scalellm_amd import kernels
    rng = np.random.default_rng(N + K)
    for M, rt, nw in ((1, 1, 2), (33, 2, 2), (70, 4, 4), (129, 1, 4), (40, 2, 4)):
        a64, w64, b64 = ref.int_inputs(rng, M, K, N, with_bias)
        a64 = a64 / 8.0                                            # gate values around +-10: the sigmoid is not saturated
        a, w = _dev(a64, bits), _dev(w64, bits)
        b = _dev(b64, bits) if with_bias else None
        full = torch.empty(M, N, dtype=a.dtype, device=DEV)
        unfused = torch.empty(M, N // 2, dtype=a.dtype, device=DEV)
        fused = torch.full((M, N // 2), float("nan"), dtype=a.dtype, device=DEV)
        with kernels.tuning(SLM_LINEAR_RT=rt, SLM_LINEAR_NW=nw):
            kernels.linear(a, w, full, b)
            kernels.silu_and_mul(unfused, full)
            info = kernels.linear_plan(a, w, fused, b, silu_mul=True)
            assert info.split_k == 1 and (info.row_tiles, info.waves) == (rt, nw)
            assert not kernels.linear(a, w, fused, b, silu_mul=True)
        assert torch.equal(full.cpu(), ref.rounded(ref.linear_ref(a64, w64, b64), bits))
        assert torch.equal(fused, unfused), (M, rt, nw)


@pytest.mark.parametrize("bits", ref.DTYPES)
def test_second_run_is_bit_identical_on_random_data(bits):
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(5)
    dt = ref.torch_dtype(bits)
    a = torch.randn(32, 4096, device=DEV, generator=g).to(dt)
    w = (torch.randn(512, 4096, device=DEV, generator=g) * 0.05).to(dt)
    c1, c2 = torch.empty(32, 512, dtype=dt, device=DEV), torch.empty(32, 512, dtype=dt, device=DEV)
    assert kernels.linear_plan(a, w, c1).split_k > 1
    kernels.linear(a, w, c1)
    kernels.linear(a, w, c2)
    assert torch.equal(c1, c2)


@pytest.mark.parametrize("bits", ref.DTYPES)
def test_deferred_consumers_equal_the_reduced_tensor(bits):
    """rms_norm, RoPE + KV append and the Gemma sandwich norm fed the slabs of a deferred dense call give the bits of
    the same consumer fed the reduced c (random data: the slabs' sum is NOT exact, the order must be the reduce's)"""
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(11)
    dt = ref.torch_dtype(bits)
    T, K, H, HKV, D = 7, 1024, 4, 2, 32
    N = (H + 2 * HKV) * D                                               # 256
    a = torch.randn(T, K, device=DEV, generator=g).to(dt)
    w = (torch.randn(N, K, device=DEV, generator=g) * 0.05).to(dt)
    nw_ = (1 + 0.1 * torch.randn(N, device=DEV, generator=g)).to(dt)
    res0 = torch.randn(T, N, device=DEV, generator=g).to(dt)
    with kernels.tuning(SLM_LINEAR_SPLITK=3):
        c = torch.empty(T, N, dtype=dt, device=DEV)
        assert not kernels.linear(a, w, c)
        unwritten = torch.full((T, N), float("nan"), dtype=dt, device=DEV)

        # RMSNorm (+ residual)
        out_a, res_a = torch.empty_like(c), res0.clone()
        kernels.rms_norm(out_a, c, nw_, 1e-5, residual=res_a)
        h = kernels.linear(a, w, unwritten, defer_reduce=True)
        assert int(h) == 3
        out_b, res_b = torch.empty_like(c), res0.clone()
        kernels.rms_norm(out_b, unwritten, nw_, 1e-5, residual=res_b, partials=h)
        assert torch.equal(out_a, out_b) and torch.equal(res_a, res_b)

        # Gemma sandwich norm
        post = (0.1 * torch.randn(N, device=DEV, generator=g)).to(dt)
        out_a, res_a = torch.empty_like(c), res0.clone()
        kernels.gemma_sandwich_norm(out_a, c, post, res_a, nw_, 1e-6)
        h = kernels.linear(a, w, unwritten, defer_reduce=True)
        out_b, res_b = torch.empty_like(c), res0.clone()
        kernels.gemma_sandwich_norm(out_b, unwritten, post, res_b, nw_, 1e-6, partials=h)
        assert torch.equal(out_a, out_b) and torch.equal(res_a, res_b)

        # RoPE + KV append over the [q | k | v] columns
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
        h = kernels.linear(a, w, buf, defer_reduce=True)
        qkv_b, kc_b, vc_b = rope(buf, h)
        assert torch.equal(qkv_a, qkv_b) and torch.equal(kc_a, kc_b) and torch.equal(vc_a, vc_b)


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M,K,N", [(1, 4096, 512), (32, 1024, 256), (160, 512, 96)])
def test_random_data_within_the_gemm_tolerance(M, K, N, bits):
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(M + N)
    dt = ref.torch_dtype(bits)
    a = torch.randn(M, K, device=DEV, generator=g).to(dt)
    w = (torch.randn(N, K, device=DEV, generator=g) * 0.05).to(dt)
    b = torch.randn(N, device=DEV, generator=g).to(dt)
    c = torch.empty(M, N, dtype=dt, device=DEV)
    kernels.linear(a, w, c, b)
    want = ref.linear_ref(ref.as64(a), ref.as64(w), ref.as64(b))
    err = ref.rel_err(ref.as64(c), want)
    print(f"[dense] {bits} M={M} K={K} N={N}: mean relative error {err:.3e} (bound {ref.GEMM_TOL[bits]:.0e})")
    assert err < ref.GEMM_TOL[bits]


def test_graph_replay_follows_the_input():
    """one split call and one SiLU call captured; the replay after overwriting `a` in place equals eager on the new a"""
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(23)
    dt = torch.bfloat16
    a = torch.randn(8, 2048, device=DEV, generator=g).to(dt)
    w = (torch.randn(256, 2048, device=DEV, generator=g) * 0.05).to(dt)
    c, cs = torch.empty(8, 256, dtype=dt, device=DEV), torch.empty(8, 128, dtype=dt, device=DEV)
    assert kernels.linear_plan(a, w, c).split_k > 1
    kernels.linear(a, w, c)                                             # warm-up: sizes the workspace
    kernels.linear(a, w, cs, silu_mul=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kernels.linear(a, w, c)
        kernels.linear(a, w, cs, silu_mul=True)
    a.copy_(torch.randn(8, 2048, device=DEV, generator=g).to(dt))
    graph.replay()
    torch.cuda.synchronize()
    got, got_s = c.clone(), cs.clone()
    kernels.linear(a, w, c)
    kernels.linear(a, w, cs, silu_mul=True)
    assert torch.equal(got, c) and torch.equal(got_s, cs)
