"""The MXFP4 weight-only linear (include/slm_hip.h section 20, csrc/dense.hip + mxfp4_cvt.h) against float64, bit for
bit where the arithmetic is exact: every e2m1 code through every nibble position under eight different block scales,
integer inputs through every kernel form, the same bits as the dense kernel on the dequantised weight, the fp32 slab of
every K slice, guard rows / columns / strides with poisoned scale padding, exactly the reported workspace, the deferred
consumers, random data within the GEMM tolerance, and graph replay."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import mxfp4_ref as ref
from . import scratch_bounds_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(x64, bits):
    return ref.rounded(x64, bits).to(DEV)


def _slabs(handle, M, N):
    """the fp32 slabs [splits, M, N] a deferred call left at the start of its buffer"""
    n = handle.splits * M * N
    assert handle.ptr == handle._keep.data_ptr() and handle.numel == M * N
    return handle._keep[:4 * n].view(torch.float32).view(handle.splits, M, N)


def _rand_w(g, N, K, e_lo=121, e_hi=133):
    """uniformly random codes, random scale bytes in [e_lo, e_hi]"""
    packed = torch.randint(0, 256, (N, K // 2), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
    scale = torch.randint(e_lo, e_hi + 1, (N, K // 32), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
    return packed, scale


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("form", ref.FORMS, ids=lambda f: f"rt{f[0]}nw{f[1]}")
def test_every_code_in_every_nibble_position(form, bits):
    """The nibble of W[n, k] is (n + k) mod 16, the scale byte of block (n, k / 32) is 114 + (n + k / 32) mod 27, A is
    one-hot at m + 128 c: C[m, n] = e2m1(code) * 2^(e - 127) exactly, by value (-0 arrives as +0 through the
    accumulator).  Every code passes through every nibble of a 16-B load, both lane halves, both loads and both
    chunks, and the eight blocks of a row carry eight different scales."""
    from scalellm_amd import kernels
    M = 128
    K = N = 256
    packed, scale = ref.code_sweep(N, K)
    codes = ref.unpack(packed)
    assert np.array_equal(codes, (np.arange(N)[:, None] + np.arange(K)[None, :]) % 16)
    val = ref.w_as64(packed, scale)                                      # [n, k], from the format's definition
    packed, scale_d = packed.to(DEV), scale.to(DEV)
    dt = ref.torch_dtype(bits)
    assert np.array_equal(ref.as64(ref.rounded(val, bits)), val)        # exact in T
    rt, nw = form
    for c in (0, 1):
        a = torch.zeros(M, K, dtype=dt, device=DEV)
        a[torch.arange(M), torch.arange(M) + 128 * c] = 1
        out = torch.full((M, N), float("nan"), dtype=dt, device=DEV)
        with kernels.tuning(**ref.knobs(rt, nw, 1)):
            info = kernels.mxfp4_linear_plan(a, packed, scale_d, out)
            assert (info.row_tiles, info.waves, info.split_k) == (rt, nw, 1)
            kernels.mxfp4_linear(a, packed, scale_d, out)
        want = val[:, 128 * c:128 * c + M].T                             # [m, n]
        got = ref.as64(out)
        bad = np.argwhere(got != want)
        if bad.size:
            m, n = bad[0]
            k = m + 128 * c
            raise AssertionError(
                f"c {c}: {len(bad)} wrong, first (m, n) = ({m}, {n}): code {codes[n, k]} in nibble {k % 32} of block "
                f"{k // 32} of row {n} (k = {k}, {'high' if k & 1 else 'low'} nibble of byte {k // 2}, scale byte "
                f"{int(scale[n, k // 32])}) gave {got[m, n]}, want {want[m, n]}")


@pytest.mark.parametrize("bits", ref.DTYPES)
def test_scale_bytes_outside_the_exact_range_behave_as_documented(bits):
    """What include/slm_hip.h section 20 says about scale bytes outside the exact range, through an ordinary call: row
    (e, code) holds `code` at k = 0 under scale byte e and zeros (e = 127) elsewhere, A is one-hot at k = 0.  For
    e < 255 the weight is the IEEE conversion of the exact product to T -- round to nearest even into the subnormals
    (kept, not flushed), +-inf beyond the largest finite number, e = 0 being 2^-127 -- and for e = 255, the MX NaN,
    NaN for every code, zero included."""
    from scalellm_amd import kernels
    dt = ref.torch_dtype(bits)
    es = [0, 1, 2, 100, 112, 113, 114, 140, 141, 142, 143, 144, 252, 253, 254, 255]
    N, K = 16 * len(es), 128
    codes = np.zeros((N, K), dtype=np.int64)
    scale = np.full((N, K // 32), 127, dtype=np.uint8)
    for i, e in enumerate(es):
        codes[16 * i:16 * i + 16, 0] = np.arange(16)
        scale[16 * i:16 * i + 16, 0] = e
    a = torch.zeros(1, K, dtype=dt, device=DEV)
    a[0, 0] = 1
    c = torch.full((1, N), 7.0, dtype=dt, device=DEV)
    with kernels.tuning(SLM_LINEAR_SPLITK=1):
        kernels.mxfp4_linear(a, ref.pack(codes).to(DEV), torch.from_numpy(scale).to(DEV), c)
    got = c.double().cpu().numpy()[0]
    for i, e in enumerate(es):
        col = got[16 * i:16 * i + 16]
        if e == 255:
            assert np.isnan(col).all(), (e, col)
            continue
        with np.errstate(over="ignore"):
            want = ref.as64(ref.rounded(ref.E2M1 * 2.0 ** (e - 127), bits))
        assert np.array_equal(col, want), (bits, e, col.tolist(), want.tolist())
        if (bits == "bf16" and 2 <= e <= 252) or (bits == "f16" and 114 <= e <= 140):
            assert np.array_equal(col, ref.E2M1 * 2.0 ** (e - 127))     # the exact range
    if bits == "bf16":
        assert got[1] == 2.0 ** -128 and np.isinf(got[16 * es.index(253) + 7])   # e = 0 is 2^-127, not 0
    else:
        assert got[16 * es.index(100) + 7] == 2.0 ** -24 and np.isinf(got[16 * es.index(141) + 6])


_CASES_BY_FORM ={f: [c for c in ref.EXACT_CASES if (c[3], c[4]) == f] for f in ref.FORMS}


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("form", ref.FORMS, ids=lambda f: f"rt{f[0]}nw{f[1]}")
def test_integer_inputs_are_exact_in_every_form(form, bits):
    """a integers in [-4, 4], W codes of {0, +-1, +-2, +-3, +-4, +-6} under block scales e in {125 .. 128}, integer
    bias: every partial sum is exact in fp32 in any order (mxfp4_ref.int_inputs), so the result is ONE rounding of the
    float64 reference"""
    from scalellm_amd import kernels
    rng = np.random.default_rng(17)
    for M, N, K, rt, nw, split, with_bias in _CASES_BY_FORM[form]:
        a64, packed, scale, b64 = ref.int_inputs(rng, M, K, N, with_bias)
        a, w, sc = _dev(a64, bits), packed.to(DEV), scale.to(DEV)
        b = _dev(b64, bits) if with_bias else None
        c = torch.full((M, N), float("nan"), dtype=a.dtype, device=DEV)
        with kernels.tuning(**ref.knobs(rt, nw, split)):
            info = kernels.mxfp4_linear_plan(a, w, sc, c, b)
            assert (info.row_tiles, info.waves, info.split_k) == (rt, nw, split)
            h = kernels.mxfp4_linear(a, w, sc, c, b)
        assert not h
        want = ref.rounded(ref.mxfp4_ref(a64, packed, scale, b64), bits)
        assert torch.equal(c.cpu(), want), (M, N, K, rt, nw, split, with_bias)


@pytest.mark.parametrize("bits", ref.DTYPES)
def test_same_bits_as_the_dense_kernel_on_the_dequantised_weight(bits):
    """random codes, random scale bytes in [121, 133], random A, the same forced (rt, nw, split): slm_mxfp4_linear(A,
    W, e) is slm_linear(A, T(dequant(W, e))) bit for bit -- the output, every slab of a deferred split, and the SiLU
    form with bias.  Pins the conversion and the accumulation order of the new weight side to the dense one's."""
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(29)
    dt = ref.torch_dtype(bits)
    for M, N, K, rt, nw, split in ref.SAME_BITS_CASES:
        a = torch.randn(M, K, device=DEV, generator=g).to(dt)
        w, sc = _rand_w(g, N, K)
        wt = kernels.dequantize_mxfp4_weight(w, sc, dt)
        assert np.array_equal(wt.double().cpu().numpy(), ref.w_as64(w, sc))   # e2m1 * 2^s -> T is exact
        with kernels.tuning(**ref.knobs(rt, nw, split)):
            c_d = torch.full((M, N), float("nan"), dtype=dt, device=DEV)
            c_4 = torch.full((M, N), float("nan"), dtype=dt, device=DEV)
            assert kernels.mxfp4_linear_plan(a, w, sc, c_4).split_k == split
            kernels.linear(a, wt, c_d)
            kernels.mxfp4_linear(a, w, sc, c_4)
            assert torch.equal(c_d, c_4), (M, N, K, rt, nw, split)
            h = kernels.linear(a, wt, c_d, defer_reduce=True)
            assert int(h) == split
            slabs_d = _slabs(h, M, N).clone()
            h = kernels.mxfp4_linear(a, w, sc, c_4, defer_reduce=True)
            assert int(h) == split
            assert torch.equal(slabs_d, _slabs(h, M, N)), (M, N, K, rt, nw, split)
    M, N, K, rt, nw, split = ref.SAME_BITS_SILU
    a = (torch.randn(M, K, device=DEV, generator=g) / 64).to(dt)       # |gate|, |up| of a few units
    w, sc = _rand_w(g, N, K)
    wt = kernels.dequantize_mxfp4_weight(w, sc, dt)
    assert np.array_equal(wt.double().cpu().numpy(), ref.w_as64(w, sc))
    bias = torch.randn(N, device=DEV, generator=g).to(dt)
    with kernels.tuning(**ref.knobs(rt, nw, split)):
        c_d = torch.full((M, N // 2), float("nan"), dtype=dt, device=DEV)
        c_4 = torch.full((M, N // 2), float("nan"), dtype=dt, device=DEV)
        info = kernels.mxfp4_linear_plan(a, w, sc, c_4, bias, silu_mul=True)
        assert (info.row_tiles, info.waves, info.split_k) == (rt, nw, 1)
        kernels.linear(a, wt, c_d, bias, silu_mul=True)
        kernels.mxfp4_linear(a, w, sc, c_4, bias, silu_mul=True)
        assert torch.equal(c_d, c_4) and not torch.isnan(c_4.float()).any()


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M,N,K,rt,nw,split", ref.SAME_BITS_CASES)
def test_every_slab_is_the_sum_over_exactly_its_slice(M, N, K, rt, nw, split, bits):
    from scalellm_amd import kernels
    rng = np.random.default_rng(M + K)
    a64, packed, scale, b64 = ref.int_inputs(rng, M, K, N, True)
    a, w, sc, b = _dev(a64, bits), packed.to(DEV), scale.to(DEV), _dev(b64, bits)
    c = torch.full((M, N), float("nan"), dtype=a.dtype, device=DEV)
    with kernels.tuning(**ref.knobs(rt, nw, split)):
        info = kernels.mxfp4_linear_plan(a, w, sc, c, None, defer_reduce=True)
        assert info.split_k == split
        h = kernels.mxfp4_linear(a, w, sc, c, None, defer_reduce=True)
        assert int(h) == split
        slabs = _slabs(h, M, N).clone()
        assert torch.isnan(c).all(), "a deferred call must not write c"
        for j in range(split):
            want = torch.from_numpy(ref.mxfp4_ref(a64, packed, scale, None, info.slice_k_range(j)).astype(np.float32))
            assert torch.equal(slabs[j].cpu(), want), f"slab {j}: k range {info.slice_k_range(j)}"
        # with a bias the flag is ignored: c is written, reduced, with the bias
        assert not kernels.mxfp4_linear(a, w, sc, c, b, defer_reduce=True)
        assert torch.equal(c.cpu(), ref.rounded(ref.mxfp4_ref(a64, packed, scale, b64), bits))


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M,N,K,rt,nw,split,silu", [(33, 96, 672, 2, 2, 1, False), (5, 32, 1312, 1, 1, 3, False),
                                                    (130, 160, 256, 4, 4, 2, False), (33, 192, 672, 2, 4, 1, True)])
def test_guard_rows_columns_and_strides(M, N, K, rt, nw, split, silu, bits):
    """lda > K, ldw > K/2, lds > K/32, ldc > N: NaN in every padding element of A and c's surroundings, 0xFF (the MX
    NaN) in every padding byte of the scale buffer -- e2m1 has no NaN code, so the scale is what can poison -- and
    0x77 (two 6.0) in the weight padding: the padding is never read into a sum and nothing outside c[:M, :n_out] is
    written"""
    from scalellm_amd import kernels
    rng = np.random.default_rng(3 * M + N)
    a64, packed, scale, b64 = ref.int_inputs(rng, M, K, N, True)
    if silu:
        a64 = a64 / 64.0
    dt = ref.torch_dtype(bits)
    n_out = N // 2 if silu else N
    nan = float("nan")
    a_buf = torch.full((M + 2, K + 24), nan, dtype=dt, device=DEV)
    w_buf = torch.full((N + 2, K // 2 + 48), 0x77, dtype=torch.uint8, device=DEV)
    s_buf = torch.full((N + 2, K // 32 + 10), 0xFF, dtype=torch.uint8, device=DEV)
    c_buf = torch.full((M + 4, n_out + 16), nan, dtype=dt, device=DEV)
    a, w, c = a_buf[1:M + 1, 8:K + 8], w_buf[1:N + 1, 16:K // 2 + 16], c_buf[2:M + 2, 8:n_out + 8]
    sc = s_buf[1:N + 1, 3:K // 32 + 3]                                  # an odd row stride from an odd offset
    a.copy_(_dev(a64, bits))
    w.copy_(packed.to(DEV))
    sc.copy_(scale.to(DEV))
    b = _dev(b64, bits)
    assert w.stride(0) > K // 2 and w.stride(0) % 16 == 0 and a.stride(0) > K and sc.stride(0) > K // 32
    with kernels.tuning(**ref.knobs(rt, nw, split)):
        info = kernels.mxfp4_linear_plan(a, w, sc, c, b, silu_mul=silu)
        assert (info.row_tiles, info.waves, info.split_k) == (rt, nw, split)
        kernels.mxfp4_linear(a, w, sc, c, b, silu_mul=silu)
    y = ref.mxfp4_ref(a64, packed, scale, b64)
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
def test_exactly_the_reported_workspace(bits):
    """one split call through the C entry in a buffer of exactly plan.workspace_bytes between guard bytes, poisoned
    beforehand: the output is bit-identical to the ordinary call, the guards are untouched, and a buffer one byte short
    is refused with the workspace status before any launch"""
    from scalellm_amd import _lib, kernels
    M, N, K, rt, nw, split = ref.SAME_BITS_CASES[0]
    g = torch.Generator(device=DEV).manual_seed(41)
    dt = ref.torch_dtype(bits)
    a = torch.randn(M, K, device=DEV, generator=g).to(dt)
    w, sc = _rand_w(g, N, K)
    bias = torch.randn(N, device=DEV, generator=g).to(dt)
    c_ref = torch.empty(M, N, dtype=dt, device=DEV)
    L = _lib.lib()
    with kernels.tuning(**ref.knobs(rt, nw, split)):
        kernels.mxfp4_linear(a, w, sc, c_ref, bias)
        c = torch.full((M, N), float("nan"), dtype=dt, device=DEV)
        args = kernels._mxfp4_args(a, w, sc, c, bias, False, False)
        info = kernels.mxfp4_linear_plan(a, w, sc, c, bias)
        n = int(info.workspace_bytes)
        assert info.split_k == split and n == split * M * N * 4
        region_byte, guard_byte = 0xFF, 0xA5                             # an fp32 NaN pattern in the region
        buf = torch.full((S.PRE_GUARD + n + S.post_guard_bytes(n),), guard_byte, dtype=torch.uint8, device=DEV)
        buf[S.PRE_GUARD:S.PRE_GUARD + n].fill_(region_byte)
        args.workspace, args.workspace_bytes = buf.data_ptr() + S.PRE_GUARD, n - 1
        torch.cuda.synchronize()
        assert L.slm_mxfp4_linear(C.byref(args), kernels._stream()) == -3   # SLM_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert torch.isnan(c).all() and bool((buf[S.PRE_GUARD:S.PRE_GUARD + n] == region_byte).all())
        args.workspace_bytes = n
        assert L.slm_mxfp4_linear(C.byref(args), kernels._stream()) == 0
        torch.cuda.synchronize()
    assert torch.equal(c, c_ref)
    assert S.guard_violations(buf, n, guard_byte) == []
    assert bool((buf[S.PRE_GUARD:S.PRE_GUARD + n] != region_byte).any())


@pytest.mark.parametrize("bits", ref.DTYPES)
def test_deferred_consumers_equal_the_reduced_tensor(bits):
    """rms_norm, RoPE + KV append and the Gemma sandwich norm fed the slabs of a deferred MXFP4 call give the bits of
    the same consumer fed the reduced c"""
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(11)
    dt = ref.torch_dtype(bits)
    T, K, H, HKV, D = 7, 1024, 4, 2, 32
    N = (H + 2 * HKV) * D                                               # 256
    a = torch.randn(T, K, device=DEV, generator=g).to(dt)
    w, sc = kernels.quantize_mxfp4_weight(torch.randn(N, K, device=DEV, generator=g) * 0.05)
    nw_ = (1 + 0.1 * torch.randn(N, device=DEV, generator=g)).to(dt)
    res0 = torch.randn(T, N, device=DEV, generator=g).to(dt)
    with kernels.tuning(SLM_LINEAR_SPLITK=3):
        c = torch.empty(T, N, dtype=dt, device=DEV)
        assert not kernels.mxfp4_linear(a, w, sc, c)
        unwritten = torch.full((T, N), float("nan"), dtype=dt, device=DEV)

        out_a, res_a = torch.empty_like(c), res0.clone()
        kernels.rms_norm(out_a, c, nw_, 1e-5, residual=res_a)
        h = kernels.mxfp4_linear(a, w, sc, unwritten, defer_reduce=True)
        assert int(h) == 3
        out_b, res_b = torch.empty_like(c), res0.clone()
        kernels.rms_norm(out_b, unwritten, nw_, 1e-5, residual=res_b, partials=h)
        assert torch.equal(out_a, out_b) and torch.equal(res_a, res_b)

        post = (0.1 * torch.randn(N, device=DEV, generator=g)).to(dt)
        out_a, res_a = torch.empty_like(c), res0.clone()
        kernels.gemma_sandwich_norm(out_a, c, post, res_a, nw_, 1e-6)
        h = kernels.mxfp4_linear(a, w, sc, unwritten, defer_reduce=True)
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
        h = kernels.mxfp4_linear(a, w, sc, buf, defer_reduce=True)
        qkv_b, kc_b, vc_b = rope(buf, h)
        assert torch.equal(qkv_a, qkv_b) and torch.equal(kc_a, kc_b) and torch.equal(vc_a, vc_b)


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M,K,N", ref.RANDOM_CASES)
def test_random_data_within_the_gemm_tolerance(M, K, N, bits):
    """randn * 0.02 weights through quantize_mxfp4_weight, with bias, against float64 over the SAME quantised weights
    (quantisation is the checkpoint's error, not the kernel's); the bound is the dense GEMM tolerance, unchanged: the
    operands the MFMA sees are exact T values.  The second run is bit-identical."""
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(M + N)
    dt = ref.torch_dtype(bits)
    a = torch.randn(M, K, device=DEV, generator=g).to(dt)
    w, sc = kernels.quantize_mxfp4_weight(torch.randn(N, K, device=DEV, generator=g) * 0.02)
    b = torch.randn(N, device=DEV, generator=g).to(dt)
    c, c2 = torch.empty(M, N, dtype=dt, device=DEV), torch.empty(M, N, dtype=dt, device=DEV)
    kernels.mxfp4_linear(a, w, sc, c, b)
    kernels.mxfp4_linear(a, w, sc, c2, b)
    want = ref.mxfp4_ref(ref.as64(a), w, sc, ref.as64(b))
    err = ref.rel_err(ref.as64(c), want)
    print(f"[mxfp4] {bits} M={M} K={K} N={N}: mean relative error {err:.3e} (bound {ref.GEMM_TOL[bits]:.0e})")
    assert err < ref.GEMM_TOL[bits]
    assert torch.equal(c, c2)


def test_graph_replay_follows_the_input():
    """one split call and one SiLU call captured; the replay after overwriting `a` in place equals eager on the new a"""
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(23)
    dt = torch.bfloat16
    a = torch.randn(8, 2048, device=DEV, generator=g).to(dt)
    w, sc = kernels.quantize_mxfp4_weight(torch.randn(256, 2048, device=DEV, generator=g) * 0.05)
    c, cs = torch.empty(8, 256, dtype=dt, device=DEV), torch.empty(8, 128, dtype=dt, device=DEV)
    assert kernels.mxfp4_linear_plan(a, w, sc, c).split_k > 1
    kernels.mxfp4_linear(a, w, sc, c)                                   # warm-up: sizes the workspace
    kernels.mxfp4_linear(a, w, sc, cs, silu_mul=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kernels.mxfp4_linear(a, w, sc, c)
        kernels.mxfp4_linear(a, w, sc, cs, silu_mul=True)
    a.copy_(torch.randn(8, 2048, device=DEV, generator=g).to(dt))
    graph.replay()
    torch.cuda.synchronize()
    got, got_s = c.clone(), cs.clone()
    kernels.mxfp4_linear(a, w, sc, c)
    kernels.mxfp4_linear(a, w, sc, cs, silu_mul=True)
    assert torch.equal(got, c) and torch.equal(got_s, cs)
