"""The fp8 x fp8 linear and its quantiser (include/slm_hip.h section 25, csrc/w8a8.hip), bit for bit where exact."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from . import scratch_bounds_cases as S
from . import w8a8_ref as ref
from .test_w4a4_exact_gpu import _padded, _slabs

pytestmark = pytest.mark.gpu
DEV = "cuda"
forms = pytest.mark.parametrize("form", ref.FORMS, ids=lambda f: f"rt{f[0]}nw{f[1]}")
dtypes = pytest.mark.parametrize("bits", ref.DTYPES)
# The step's checkpoint seed, and the share of rows on which _restated_ids with fake-quantised inputs picks the token
# it picks without, computed on the CPU: seeds 1 .. 6 give 1.0, 0.75, 1.0, 0.875, 0.75, 1.0; seed 1 agrees on every row
SEED, SHARE = 1, 1.0
_pad8 = lambda t, pad: _padded(t.view(torch.uint8), pad, 16).view(torch.float8_e4m3fn)  # noqa: E731 (0xFF = NaN around)


@dtypes
@pytest.mark.parametrize("swapped", [False, True], ids=["hotA", "hotW"])
@forms
def test_operand_layout_by_one_hot_sweeps(form, swapped, bits):
    """K = 160 (a chunk + a one-unit tail): one operand one-hot at k = row % 32 + o, the other every code at every k"""
    from scalellm_amd import kernels
    M, N, K = 40, 64, 160
    a_scale, w_scale = (torch.from_numpy(2.0 ** (np.arange(n) % p - 3)).float() for n, p in ((M, 5), (N, 7)))
    for o in range(0, K, 32):
        aq, w8 = ref.one_hot(M, K, o), ref.code_sweep_weight(N, K).view(torch.float8_e4m3fn)
        if swapped:
            aq, w8 = ref.code_sweep_weight(M, K).view(torch.float8_e4m3fn), ref.one_hot(N, K, o)
        want = ref.rounded(ref.w8a8_ref(aq, a_scale, w8, w_scale), bits)
        c = torch.full((M, N), float("nan"), dtype=want.dtype, device=DEV)
        with kernels.tuning(**ref.knobs(*form, 1)):
            kernels.w8a8_linear(_pad8(aq, 32), a_scale.to(DEV), _pad8(w8, 48), w_scale.to(DEV), c)
        assert torch.equal(c.cpu(), want), (o, np.argwhere((c.cpu() != want).numpy())[:4])


@dtypes
@forms
def test_integer_inputs_are_exact_in_every_form(form, bits):
    """ONE rounding of float64, also through padded strides, NaN around c and exactly plan.workspace_bytes between guards;
    slab j is the scaled sum over its k range; SiLU * mul (the first 64 weight rows) is the plain call + silu_and_mul"""
    from scalellm_amd import _lib, kernels
    rng, dt = np.random.default_rng(17), ref.torch_dtype(bits)
    for M, N, K, split in ref.INT_CASES:
        aq, asc, w8, wsc, b64 = ref.int_inputs(rng, M, K, N)
        dev = dict(aq=aq.to(DEV), a_scale=asc.to(DEV), w8=w8.to(DEV), w_scale=wsc.to(DEV))
        bias, c = ref.rounded(b64, bits).to(DEV), torch.full((M, N), float("nan"), dtype=dt, device=DEV)
        c_buf = torch.full((M + 4, N + 16), float("nan"), dtype=dt, device=DEV)
        fenced, n = c_buf[2:M + 2, 8:N + 8], split * M * N * 4 * (split > 1)
        with kernels.tuning(**ref.knobs(*form, split)):
            info = kernels.w8a8_linear_plan(c=c, **dev)
            assert (info.row_tiles, info.waves, info.split_k, info.workspace_bytes) == (*form, split, n)
            assert not kernels.w8a8_linear(c=c, bias=bias, **dev)
            assert torch.equal(c.cpu(), ref.rounded(ref.w8a8_ref(aq, asc, w8, wsc, b64), bits)), (M, N, K, split)
            args = kernels._w8a8_args(_pad8(aq, 32), dev["a_scale"], _pad8(w8, 48), dev["w_scale"], fenced, bias, False, False)
            buf = torch.full((S.PRE_GUARD + n + S.post_guard_bytes(n),), 0xA5, dtype=torch.uint8, device=DEV)
            args.workspace, args.workspace_bytes = buf.data_ptr() + S.PRE_GUARD, n
            assert _lib.lib().slm_w8a8_linear(C.byref(args), kernels._stream()) == 0 and torch.equal(fenced, c)
            fenced.fill_(float("nan"))
            assert torch.isnan(c_buf).all() and S.guard_violations(buf, n, 0xA5) == []
            if N >= 64:
                cs, want = torch.empty(M, 32, dtype=dt, device=DEV), torch.empty(M, 32, dtype=dt, device=DEV)
                kernels.w8a8_linear(dev["aq"], dev["a_scale"], dev["w8"][:64], dev["w_scale"][:64], cs, bias[:64], silu_mul=True)
                kernels.silu_and_mul(want, c[:, :64].contiguous())
                assert torch.equal(cs, want) and torch.isfinite(cs.float()).all()
            if split > 1:
                h = kernels.w8a8_linear(c=c, defer_reduce=True, **dev)
                for j in range(split):
                    want = ref.w8a8_ref(aq, asc, w8, wsc, None, info.slice_k_range(j)).astype(np.float32)
                    assert int(h) == split and torch.equal(_slabs(h, M, N)[j].cpu(), torch.from_numpy(want)), (M, N, K, j)


@dtypes
@pytest.mark.parametrize("static", [None, 0.37], ids=["dynamic", "static"])
@pytest.mark.parametrize("M,K", [(1, 32), (33, 672), (3, 8192)])
def test_the_quantiser_is_the_torch_statement(M, K, static, bits):
    """row 0: amax exactly 448, ties, e4m3 subnormals, -0; (M > 2) a zero row, a row with one inf; 0xA5 padding untouched"""
    from scalellm_amd import kernels
    dt = ref.torch_dtype(bits)
    a = (torch.randn(M, K, generator=torch.Generator().manual_seed(M + K)) * torch.logspace(-3, 3, M).view(M, 1)).to(dt)
    a[0] = torch.tensor([448.0, -1e-6, 1.0625, 1.1875, -1.0625, 2.0 ** -9 * 1.5, 2.0 ** -10, -2.0 ** -10, 2.0 ** -10 * 1.0078125,
                         -447.0, 0.0, -0.0, 300.0, 17.0, 0.0146484375, -240.0] * (K // 16)).to(dt)
    if M > 2:
        a[1], a[2, 5] = 0, float("inf")
    aq = _padded(torch.zeros(M, K, dtype=torch.uint8), 48, 16, fill=0xA5)
    _, a_scale = kernels.quantize_fp8_act(_padded(a, 24, 8, fill=float("nan"), dtype=dt),
                                          None if static is None else torch.tensor([static], device=DEV), aq=aq)
    want_q, want_s = ref.quant_ref(a, static)
    assert torch.equal(a_scale.cpu().view(torch.int32), want_s.view(torch.int32))
    assert torch.equal(aq.cpu(), want_q), np.argwhere((aq.cpu() != want_q).numpy())[:4]
    aq.fill_(0xA5)
    assert bool((aq._base == 0xA5).all())


@dtypes
@pytest.mark.parametrize("M,K,N", [(1, 1024, 256), (33, 672, 160), (129, 1312, 96)])
def test_random_data_within_the_gemm_tolerance(M, K, N, bits):
    """float64 over the SAME quantised operands (quantisation is not the kernel's error): the project's bound, unchanged"""
    from scalellm_amd import kernels
    g, dt = torch.Generator(device=DEV).manual_seed(M + N), ref.torch_dtype(bits)
    aq, asc = kernels.quantize_fp8_act(torch.randn(M, K, device=DEV, generator=g).to(dt))
    w8, wsc = kernels.quantize_fp8_weight(torch.randn(N, K, device=DEV, generator=g) * 0.02)
    b, c = torch.randn(N, device=DEV, generator=g).to(dt), torch.empty(M, N, dtype=dt, device=DEV)
    kernels.w8a8_linear(aq, asc, w8, wsc, c, b)
    err = ref.rel_err(ref.as64(c), ref.w8a8_ref(aq, asc, w8, wsc, ref.as64(b)))
    assert err <= ref.GEMM_TOL[bits], f"mean relative error {err:.3e}"


@dtypes
def test_rms_norm_over_the_slabs_equals_rms_norm_over_the_reduced_tensor(bits):
    from scalellm_amd import kernels
    g, dt, (T, K, N) = torch.Generator(device=DEV).manual_seed(11), ref.torch_dtype(bits), (7, 1024, 256)
    aq, asc = kernels.quantize_fp8_act(torch.randn(T, K, device=DEV, generator=g).to(dt))
    w8, wsc = kernels.quantize_fp8_weight(torch.randn(N, K, device=DEV, generator=g) * 0.05)
    nw_, res_a = (1 + 0.1 * torch.randn(N, device=DEV, generator=g)).to(dt), torch.randn(T, N, device=DEV, generator=g).to(dt)
    res_b, c, unwritten = res_a.clone(), torch.empty(T, N, dtype=dt, device=DEV), torch.full((T, N), float("nan"), dtype=dt, device=DEV)
    out_a, out_b = torch.empty_like(c), torch.empty_like(c)
    with kernels.tuning(SLM_W8A8_SPLITK=3):
        assert not kernels.w8a8_linear(aq, asc, w8, wsc, c)
        kernels.rms_norm(out_a, c, nw_, 1e-5, residual=res_a)
        h = kernels.w8a8_linear(aq, asc, w8, wsc, unwritten, defer_reduce=True)
        kernels.rms_norm(out_b, unwritten, nw_, 1e-5, residual=res_b, partials=h)
    assert int(h) == 3 and torch.equal(out_a, out_b) and torch.equal(res_a, res_b) and torch.isnan(unwritten).all()


@dtypes
def test_the_layers_run_the_w8a8_kernel(bits):
    from scalellm_amd import kernels
    from scalellm_amd.layers import ColumnParallelFp8Linear
    from scalellm_amd.model_parallel import ParallelArgs
    g, dt, pa = torch.Generator(device=DEV).manual_seed(2), ref.torch_dtype(bits), ParallelArgs(rank=0, world_size=1)
    parts = [kernels.quantize_fp8_weight(torch.randn(n, 672, device=DEV, generator=g) * 0.05, per="tensor") for n in (64, 32, 32)]
    x = torch.randn(9, 672, device=DEV, generator=g).to(dt)
    want, w8a16 = torch.empty(9, 128, dtype=dt, device=DEV), torch.empty(9, 128, dtype=dt, device=DEV)
    for scale in (None, torch.tensor([0.011], device=DEV)):
        sd = {f"{p}_proj.weight{s}": t for p, ws in zip("qkv", parts) for s, t in zip(("", "_scale"), (ws[0], ws[1][:1]))}
        sd.update({} if scale is None else {"q_proj.input_scale": scale.cpu(), "k_proj.input_scale": scale.cpu() / 2})
        qkv, old = (ColumnParallelFp8Linear(672, 128, False, False, pa, dt, DEV, act_quant=q) for q in ("fp8", None))
        for lin in (qkv, old):
            lin.load_state_dict(dict(sd), ["q_proj.", "k_proj.", "v_proj."])
        assert torch.equal(qkv.weight_scale, torch.cat([s for _, s in parts])) and old.input_scale is None
        aq, asc = kernels.quantize_fp8_act(x, scale)
        assert scale is None or (torch.equal(qkv.input_scale, scale) and bool((asc == scale).all()))
        kernels.w8a8_linear(aq, asc, qkv.weight, qkv.weight_scale, want)
        kernels.fp8_linear(x, old.weight, old.weight_scale, w8a16)
        assert torch.equal(qkv.forward(x), want) and torch.equal(old.forward(x), w8a16) and not torch.equal(want, w8a16)


def _composed(model, tokens, positions, params):
    from scalellm_amd import kernels   # the step's logits from its layers' forward calls, one launch after the other
    s, T = model.shape, tokens.numel()
    nq, nkv = model.n_heads * s.head_dim, model.n_kv_heads * s.head_dim
    resid = model.embed[tokens.long()].clone()
    normed, attn = torch.empty_like(resid), torch.empty(T, model.n_heads, s.head_dim, dtype=resid.dtype, device=DEV)
    kernels.rms_norm(normed, resid, model.layers[0]["in_norm"], s.rms_eps)
    for li, L in enumerate(model.layers):
        qkv = L["qkv"].forward(normed)
        q = model.attn.append(qkv[:, :nq], qkv[:, nq:nq + nkv], qkv[:, nq + nkv:], positions, L["kv"], params)
        model.attn.decode(q, L["kv"], params, output=attn)
        kernels.rms_norm(normed, L["o"].forward(attn.view(T, -1)), L["post_norm"], s.rms_eps, residual=resid)
        delta = L["down"].forward(L["gate_up"].forward(normed))
        nxt = model.final_norm if li + 1 == len(model.layers) else model.layers[li + 1]["in_norm"]
        kernels.rms_norm(normed, delta, nxt, s.rms_eps, residual=resid)
    return normed[(params.q_cu_seq_lens[1:] - 1).long()] @ model.lm_head


def _restated_ids(model, tokens, fake_quant):
    """A NARROW restatement: torch fp32 on the CPU over the kept checkpoint, valid only for sequences at their first
    token (one visible key: the attention output is v).  fake_quant: each linear's input through section 25's rule."""
    f = lambda t: t.float().cpu()  # noqa: E731
    s, T = model.shape, tokens.numel()

    def lin(x, ck):
        if fake_quant:
            codes, sc = ref.quant_ref(x)
            x = codes.view(torch.float8_e4m3fn).float() * sc[:, None]
        return x @ (f(ck["weight"]) * f(ck["weight_scale"])[:, None]).t()

    def norm(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + s.rms_eps) * f(w)
    h = f(model.embed)[tokens.cpu().long()]
    for L, ck in zip(model.layers, model.ckpt):
        v = lin(norm(h, L["in_norm"]), ck["qkv"])[:, (s.n_heads + s.n_kv_heads) * s.head_dim:]
        v = v.view(T, s.n_kv_heads, 1, s.head_dim).expand(-1, -1, s.n_heads // s.n_kv_heads, -1).reshape(T, -1)
        h = h + lin(v, ck["o"])
        gu = lin(norm(h, L["post_norm"]), ck["gate_up"])
        h = h + lin(torch.nn.functional.silu(gu[:, :s.intermediate]) * gu[:, s.intermediate:], ck["down"])
    return (norm(h, model.final_norm) @ f(model.lm_head)).argmax(-1)


def test_the_llama_step_with_fp8_activations():
    """logits: the composed layers' bits, eager, repeated, replayed; ids: agree with act_quant=None where _restated_ids does"""
    from scalellm_amd.model_runner import ModelRunner, ModelRunnerOptions
    from tests.test_dense_step_gpu import _filled
    from tests.test_model_runner_gpu import _batch
    from tests.test_mxfp4_step_gpu import LINEARS, _step
    B, max_len, n_blocks, bs = 16, 496, 400, 8
    model, w8a16 = (_step("fp8", bs, n_blocks, B, seed=SEED, keep_checkpoint=True, **kw) for kw in ({"act_quant": "fp8"}, {}))
    assert all(L[n].act_quant == "fp8" and M[n].act_quant is None for L, M in zip(model.layers, w8a16.layers) for n in LINEARS)
    restore, rng = _filled(model, 11), np.random.default_rng(5)
    runner = ModelRunner(model, model.device, ModelRunnerOptions(block_size=B, cuda_graph_max_seq_len=max_len,
                                                        cuda_graph_batch_sizes=[bs], num_decoding_tokens=1), return_logits=True)
    runner.capture_cuda_graphs(bs)
    for trial in range(2):
        kv = [int(x) for x in rng.integers(1 + 100 * trial, 150 + 100 * trial, size=bs)]
        t2, p2, prm2 = _batch(rng, bs, 1, kv, B, n_blocks, model.shape.vocab)
        hinted = dataclasses.replace(prm2, kv_max_seq_len=max_len)
        restore()
        want = _composed(model, t2, p2, hinted)
        assert torch.isfinite(want.float()).all() and all(torch.isfinite(L["kv"].key_cache.float()).all() for L in model.layers)
        for run in (lambda: model.forward(t2, p2, hinted, return_logits=True),) * 2 + (lambda: runner.forward(t2, p2, prm2),):
            restore()
            assert torch.equal(run(), want)
    t1, p1, prm1 = _batch(np.random.default_rng(SEED), bs, 1, [1] * bs, B, n_blocks, model.shape.vocab)
    share = float((_restated_ids(model, t1, True) == _restated_ids(model, t1, False)).float().mean())
    got = float((model.forward(t1, p1, prm1) == w8a16.forward(t1, p1, prm1)).float().mean())
    print(f"[w8a8 step] seed {SEED}: restated share {share:.3f}, W8A8 against W8A16 on the GPU {got:.3f}")
    assert share == SHARE and got >= share
