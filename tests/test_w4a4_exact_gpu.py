"""The MXFP4 x MXFP4 linear (include/slm_hip.h section 22, csrc/w4a4.hip + w4a4_quant.h) against float64, bit for bit
where the arithmetic is exact: the scaled MFMA's operand layout by one-hot sweeps, the quantiser against
quantize_mxfp4_weight, integer inputs through every form, the T side against quantiser + pre-quantised side, guards,
random data within the GEMM tolerance, the deferred consumer, the layers and the Llama step."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from . import scratch_bounds_cases as S
from . import w4a4_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
forms = pytest.mark.parametrize("form", ref.FORMS, ids=lambda f: f"rt{f[0]}nw{f[1]}")
dtypes = pytest.mark.parametrize("bits", ref.DTYPES)


def _slabs(handle, M, N):
    return handle._keep[:4 * handle.splits * M * N].view(torch.float32).view(handle.splits, M, N)


def _padded(t, pad_cols, lead, fill=0xFF, dtype=torch.uint8):
    """`t` as a view into a larger buffer filled with `fill`: one guard row above and below, `lead` columns in front"""
    buf = torch.full((t.size(0) + 2, t.size(1) + pad_cols), fill, dtype=dtype, device=DEV)
    buf[1:-1, lead:lead + t.size(1)] = t.to(DEV)
    return buf[1:-1, lead:lead + t.size(1)]


@dtypes
@pytest.mark.parametrize("swapped", [False, True], ids=["hotA", "hotW"])
@forms
def test_operand_layout_by_one_hot_sweeps(form, swapped, bits):
    """One operand is one-hot (1.0 at k = row % 32 + o, o = 0, 32 .. 256: two chunks and a one-unit tail), the other
    ref.code_sweep: every code passes through every k of a chunk and of the tail unit, on either operand, and the scale
    bytes differ per (row, block) on both, through padded strides and an odd scale base.  C[m, n] is one product."""
    from scalellm_amd import kernels
    M, N, K = 32, 64, 288
    for o in range(0, K, 32):
        (aq, asc), (wq, wsc) = ref.one_hot(M, K, o), ref.code_sweep(N, K)
        if swapped:
            (aq, asc), (wq, wsc) = ref.code_sweep(M, K), ref.one_hot(N, K, o)
        want = ref.rounded(ref.w4a4_ref(aq, asc, wq, wsc), bits)
        c = torch.full((M, N), float("nan"), dtype=want.dtype, device=DEV)
        with kernels.tuning(**ref.knobs(*form, 1)):
            kernels.w4a4_linear(_padded(aq, 32, 16), _padded(wq, 48, 16), _padded(wsc, 10, 3), c, a_scale=_padded(asc, 6, 1))
        bad = np.argwhere((c.cpu() != want).numpy())
        assert not bad.size, f"o {o}: {len(bad)} wrong, first (m, n) = {bad[0]}: {c[tuple(bad[0])]} != {want[tuple(bad[0])]}"


@dtypes
@pytest.mark.parametrize("M,K", [(1, 32), (33, 32), (1, 672), (33, 672)])
def test_the_quantiser_follows_quantize_mxfp4_weight(M, K, bits):
    """random blocks over many magnitudes, then one block each of: every midpoint between grid points and values beyond
    6 (under scales 2^0 and 2^-9), zeros, the clamp ends (only bf16 reaches them), f16 subnormals, an inf (e = 255)"""
    from scalellm_amd import kernels
    dt, nb = ref.torch_dtype(bits), K // 32
    g = torch.Generator().manual_seed(M + K)
    a = (torch.randn(M, nb, 32, generator=g) * torch.logspace(-5, 4, M * nb).view(M, nb, 1)).view(M, K).to(dt)
    mid = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -2.5, -5.0, 7.0, 7.5, -7.9, 6.0, 4.0, -0.24, 0.26,
                        -1.26, 3.49, 2.51, 4.99, 5.01] + [0.0] * 10)
    blocks = [mid, mid * 2.0 ** -9, torch.zeros(32), torch.full((32,), 2.0 ** -130), torch.arange(32) * 2.0 ** -24,
              torch.full((32,), 2.0 ** 127 * 1.5 if bits == "bf16" else 49152.0), torch.tensor([float("inf")] + [1.0] * 31)]
    where = [((i * 5) % M, (i * 4) % nb) for i in range(min(len(blocks), M * nb))]
    for (r, kb), b in zip(where, blocks):
        a[r, 32 * kb:32 * kb + 32] = b.to(dt)
    aq, asc = (t.cpu() for t in kernels.quantize_mxfp4_act(_padded(a, 24, 8, fill=float("nan"), dtype=dt)))
    if len(where) == len(blocks):   # the inf block: e = 255; compared as a block of ones
        r, kb = where[-1]
        assert asc[r, kb] == 255
        a[r, 32 * kb:32 * kb + 32], asc[r, kb], aq[r, 16 * kb:16 * kb + 16] = 1.0, 125, 0x66
    wq, wsc = kernels.quantize_mxfp4_weight(a.float())
    got, want = ref.unpack(aq), ref.unpack(wq)
    got[got == 8] = 0
    assert torch.equal(asc, wsc) and np.array_equal(got, want), np.argwhere(got != want)[:4]


@dtypes
@forms
def test_integer_inputs_are_exact_in_every_form(form, bits):
    """ref.int_inputs: every partial sum is exact in fp32 in any order, so the output is ONE rounding of float64 and a
    deferred split's slab j is exactly the sum over its k range; SiLU * mul is the plain call + silu_and_mul"""
    from scalellm_amd import kernels
    rng = np.random.default_rng(17)
    dt = ref.torch_dtype(bits)
    silu_case = [(33, 128, 672, *form, 1, True)] if form[1] >= 2 else []
    for M, N, K, rt, nw, split, with_bias in [c for c in ref.EXACT_CASES if c[3:5] == form] + silu_case:
        silu = N == 128
        aq, asc, wq, wsc, b64 = ref.int_inputs(rng, M, K, N, with_bias)
        asc = asc - 5 if silu else asc                                  # |gate|, |up| of a few units
        dev = dict(a=aq.to(DEV), w=wq.to(DEV), w_scale=wsc.to(DEV), a_scale=asc.to(DEV),
                   bias=ref.rounded(b64, bits).to(DEV) if with_bias else None)
        c = torch.full((M, N), float("nan"), dtype=dt, device=DEV)
        with kernels.tuning(**ref.knobs(rt, nw, split)):
            info = kernels.w4a4_linear_plan(c=c, **dev)
            assert (info.row_tiles, info.waves, info.split_k) == (rt, nw, split)
            assert not kernels.w4a4_linear(c=c, **dev)
            assert torch.equal(c.cpu(), ref.rounded(ref.w4a4_ref(aq, asc, wq, wsc, b64), bits)), (M, N, K, split)
            if split > 1 and not with_bias:
                h = kernels.w4a4_linear(c=c, defer_reduce=True, **dev)
                assert int(h) == split
                for j in range(split):
                    want = ref.w4a4_ref(aq, asc, wq, wsc, None, info.slice_k_range(j)).astype(np.float32)
                    assert torch.equal(_slabs(h, M, N)[j].cpu(), torch.from_numpy(want)), (M, N, K, j)
            if silu:
                cs, want = torch.empty(M, N // 2, dtype=dt, device=DEV), torch.empty(M, N // 2, dtype=dt, device=DEV)
                kernels.w4a4_linear(c=cs, silu_mul=True, **dev)
                kernels.silu_and_mul(want, c)
                assert torch.equal(cs, want)


@dtypes
@forms
def test_the_t_side_is_the_quantiser_then_the_prequantised_side(form, bits):
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(5)
    dt = ref.torch_dtype(bits)
    for M, N, K, split in ref.CORNERS + (((33, 128, 672, 1),) if form[1] >= 2 else ()):
        silu = N == 128
        a = (torch.randn(M, K, device=DEV, generator=g) * (0.1 if silu else 3.0)).to(dt)
        w, sc = kernels.quantize_mxfp4_weight(torch.randn(N, K, device=DEV, generator=g) * 0.05)
        aq, asc = kernels.quantize_mxfp4_act(a)
        c_t = torch.full((M, N // 2 if silu else N), float("nan"), dtype=dt, device=DEV)
        c_q = c_t.clone()
        with kernels.tuning(**ref.knobs(*form, split)):
            kernels.w4a4_linear(a, w, sc, c_t, silu_mul=silu)
            kernels.w4a4_linear(aq, w, sc, c_q, silu_mul=silu, a_scale=asc)
        assert torch.equal(c_t, c_q) and torch.isfinite(c_t.float()).all(), (M, N, K, split)


@dtypes
@pytest.mark.parametrize("quantised", [False, True], ids=["T", "prequantised"])
@pytest.mark.parametrize("M,N,K,rt,nw,split", [(33, 96, 672, 2, 2, 1), (5, 32, 1312, 1, 1, 3), (130, 160, 160, 4, 4, 1)])
def test_guard_rows_columns_strides_and_exactly_the_workspace(M, N, K, rt, nw, split, quantised, bits):
    """partial row tile / NW group, padded lda / ldas / ldw / lds / ldc with 0xFF (the MX NaN where it is a scale, NaN
    where it is T) in every padding byte, NaN around c, the workspace exactly plan.workspace_bytes between guards"""
    from scalellm_amd import _lib, kernels
    aq, asc, wq, wsc, b64 = ref.int_inputs(np.random.default_rng(3 * M + N), M, K, N, True)
    dt = ref.torch_dtype(bits)
    if quantised:
        a, a_scale = _padded(aq, 32, 16), _padded(asc, 7, 3)
    else:   # values on the grid with a 6 in every block quantise back to themselves
        aq[:, 0::16] = (aq[:, 0::16] & 0xF0) | 7
        a, a_scale = _padded(ref.rounded(ref.w_as64(aq, asc), bits), 24, 8, fill=float("nan"), dtype=dt), None
    w, sc, b = _padded(wq, 48, 16), _padded(wsc, 10, 3), ref.rounded(b64, bits).to(DEV)
    c_buf = torch.full((M + 4, N + 16), float("nan"), dtype=dt, device=DEV)
    c = c_buf[2:M + 2, 8:N + 8]
    with kernels.tuning(**ref.knobs(rt, nw, split)):
        args = kernels._w4a4_args(a, a_scale, w, sc, c, b, False, False)
        info = kernels.w4a4_linear_plan(a, w, sc, c, b, a_scale=a_scale)
        n = int(info.workspace_bytes)
        assert (info.row_tiles, info.waves, info.split_k) == (rt, nw, split) and n == (split * M * N * 4 if split > 1 else 0)
        buf = torch.full((S.PRE_GUARD + n + S.post_guard_bytes(n),), 0xA5, dtype=torch.uint8, device=DEV)
        args.workspace, args.workspace_bytes = buf.data_ptr() + S.PRE_GUARD, n
        assert _lib.lib().slm_w4a4_linear(C.byref(args), kernels._stream()) == 0
        torch.cuda.synchronize()
    assert torch.equal(c.cpu(), ref.rounded(ref.w4a4_ref(aq, asc, wq, wsc, b64), bits))
    c_buf[2:M + 2, 8:N + 8] = float("nan")
    assert torch.isnan(c_buf).all() and S.guard_violations(buf, n, 0xA5) == []


@dtypes
@pytest.mark.parametrize("M,K,N", [(1, 1024, 256), (33, 672, 160), (129, 1312, 96)])
def test_random_data_within_the_gemm_tolerance(M, K, N, bits):
    """randn A through the T side against float64 over the SAME quantised operands (quantisation is not the kernel's
    error): the project's fp32-accumulation bound, unchanged.  The second run is bit-identical."""
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(M + N)
    dt = ref.torch_dtype(bits)
    a = torch.randn(M, K, device=DEV, generator=g).to(dt)
    w, sc = kernels.quantize_mxfp4_weight(torch.randn(N, K, device=DEV, generator=g) * 0.02)
    b = torch.randn(N, device=DEV, generator=g).to(dt)
    c, c2 = torch.empty(M, N, dtype=dt, device=DEV), torch.empty(M, N, dtype=dt, device=DEV)
    kernels.w4a4_linear(a, w, sc, c, b)
    kernels.w4a4_linear(a, w, sc, c2, b)
    err = ref.rel_err(ref.as64(c), ref.w4a4_ref(*kernels.quantize_mxfp4_act(a), w, sc, ref.as64(b)))
    print(f"[w4a4] {bits} M={M} K={K} N={N}: mean relative error {err:.3e} (bound {ref.GEMM_TOL[bits]:.0e})")
    assert err < ref.GEMM_TOL[bits] and torch.equal(c, c2)


@dtypes
def test_rms_norm_over_the_slabs_equals_rms_norm_over_the_reduced_tensor(bits):
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(11)
    dt, (T, K, N) = ref.torch_dtype(bits), (7, 1024, 256)
    a = torch.randn(T, K, device=DEV, generator=g).to(dt)
    w, sc = kernels.quantize_mxfp4_weight(torch.randn(N, K, device=DEV, generator=g) * 0.05)
    nw_ = (1 + 0.1 * torch.randn(N, device=DEV, generator=g)).to(dt)
    res_a = torch.randn(T, N, device=DEV, generator=g).to(dt)
    res_b, c, unwritten = res_a.clone(), torch.empty(T, N, dtype=dt, device=DEV), torch.full((T, N), float("nan"), dtype=dt, device=DEV)
    out_a, out_b = torch.empty_like(c), torch.empty_like(c)
    with kernels.tuning(SLM_W4A4_SPLITK=3):
        assert not kernels.w4a4_linear(a, w, sc, c)
        kernels.rms_norm(out_a, c, nw_, 1e-5, residual=res_a)
        h = kernels.w4a4_linear(a, w, sc, unwritten, defer_reduce=True)
        assert int(h) == 3
        kernels.rms_norm(out_b, unwritten, nw_, 1e-5, residual=res_b, partials=h)
    assert torch.equal(out_a, out_b) and torch.equal(res_a, res_b) and torch.isnan(unwritten).all()


@dtypes
def test_the_layers_run_the_w4a4_kernel(bits):
    from scalellm_amd import kernels
    from scalellm_amd.layers import ColumnParallelMxfp4Linear, RowParallelMxfp4Linear
    from scalellm_amd.model_parallel import ParallelArgs
    g = torch.Generator(device=DEV).manual_seed(2)
    dt, pa = ref.torch_dtype(bits), ParallelArgs(rank=0, world_size=1)
    parts = [kernels.quantize_mxfp4_weight(torch.randn(n, 672, device=DEV, generator=g) * 0.05) for n in (64, 32, 32)]
    qkv = ColumnParallelMxfp4Linear(672, 128, False, False, pa, dt, DEV, act_quant="mxfp4")
    qkv.load_state_dict({f"{p}_proj.weight{s}": t for p, ws in zip("qkv", parts) for s, t in zip(("", "_scale"), ws)},
                        ["q_proj.", "k_proj.", "v_proj."])
    assert torch.equal(qkv.weight_scale, torch.cat([s for _, s in parts]))   # each shard keeps its scales
    row = RowParallelMxfp4Linear(672, 64, True, True, pa, dt, DEV, act_quant="mxfp4")
    row.load_shard(*parts[0], torch.randn(64, device=DEV, generator=g).to(dt))
    x = torch.randn(9, 672, device=DEV, generator=g).to(dt)
    for lin in (qkv, row):
        want, w4a16 = torch.empty(9, lin.local_out, dtype=dt, device=DEV), torch.empty(9, lin.local_out, dtype=dt, device=DEV)
        kernels.w4a4_linear(x, lin.weight, lin.weight_scale, want, lin.bias)
        kernels.mxfp4_linear(x, lin.weight, lin.weight_scale, w4a16, lin.bias)
        assert torch.equal(lin.forward(x), want) and not torch.equal(want, w4a16)
    with pytest.raises(ValueError, match="act_quant"):
        ColumnParallelMxfp4Linear(672, 128, False, False, pa, dt, DEV, act_quant="fp8")


def test_the_llama_step_with_mxfp4_activations():
    """every linear is the W4A4 layer; a captured graph's replay on new inputs equals eager; repeats are bit-identical;
    the appended KV is finite.  The greedy-token agreement with the W4A16 step is printed: activation quantisation is
    the checkpoint's numerics, not a kernel error."""
    from scalellm_amd.model_runner import ModelRunner, ModelRunnerOptions
    from tests.test_dense_step_gpu import _filled
    from tests.test_model_runner_gpu import _batch
    from tests.test_mxfp4_step_gpu import DEV as dev, LINEARS, _step
    B, max_len, n_blocks, bs = 16, 496, 400, 8
    model, w4a16 = _step("mxfp4", bs, n_blocks, B, seed=1, act_quant="mxfp4"), _step("mxfp4", bs, n_blocks, B, seed=1)
    assert all(L[n].act_quant == "mxfp4" and M[n].act_quant is None for L, M in zip(model.layers, w4a16.layers) for n in LINEARS)
    with pytest.raises(ValueError, match="act_quant"):
        _step("fp8", bs, n_blocks, B, act_quant="mxfp4")
    restore, restore16 = _filled(model, 11), _filled(w4a16, 11)
    rng = np.random.default_rng(5)
    runner = ModelRunner(model, dev, ModelRunnerOptions(block_size=B, cuda_graph_max_seq_len=max_len,
                                                        cuda_graph_batch_sizes=[bs], num_decoding_tokens=1), return_logits=True)
    runner.capture_cuda_graphs(bs)
    restore()
    for trial in range(2):
        kv = [int(x) for x in rng.integers(1 + 100 * trial, 150 + 100 * trial, size=bs)]
        t2, p2, prm2 = _batch(rng, bs, 1, kv, B, n_blocks, model.shape.vocab)
        hinted = dataclasses.replace(prm2, kv_max_seq_len=max_len)
        want = model.forward(t2, p2, hinted, return_logits=True).clone()
        assert all(torch.isfinite(L["kv"].key_cache.float()).all() for L in model.layers)
        restore()
        assert torch.equal(model.forward(t2, p2, hinted, return_logits=True), want)
        restore()
        assert torch.equal(runner.forward(t2, p2, prm2), want) and torch.isfinite(want.float()).all()
        restore()
        other = w4a16.forward(t2, p2, hinted, return_logits=True)
        restore16()
        print(f"[w4a4 step] trial {trial}: greedy tokens agreeing with W4A16: "
              f"{float((other.argmax(-1) == want.argmax(-1)).float().mean()):.2f}")
