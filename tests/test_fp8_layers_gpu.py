"""The fp8 weight-only linear LAYERS (layers.ColumnParallelFp8Linear / RowParallelFp8Linear and their C++ twins
slm::{Column,Row}ParallelFp8LinearHipImpl) on the GPU: against float64 over the same e4m3 weights, the fused gate | up
layer with two per-tensor scales against the plain call + silu_and_mul, tensor-parallel shards of one layer run in
turn on the one GPU, and the shim classes bit for bit against the Python classes."""
import pytest
import torch

from . import fp8_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pa(rank=0, world=1):
    from scalellm_amd.model_parallel import ParallelArgs
    return ParallelArgs(rank=rank, world_size=world)


def _tensors(bits, K, N, M, seed, per="channel"):
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(seed)
    dt = ref.torch_dtype(bits)
    w8, scale = kernels.quantize_fp8_weight(torch.randn(N, K, device=DEV, generator=g) * 0.05, per=per)
    b = torch.randn(N, device=DEV, generator=g).to(dt)
    x = torch.randn(M, K, device=DEV, generator=g).to(dt)
    return w8, scale, b, x


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M", [1, 40])
def test_python_layers_against_float64(M, bits):
    from scalellm_amd import kernels
    from scalellm_amd.layers import ColumnParallelFp8Linear, RowParallelFp8Linear
    K, N = 1024, 384
    w8, scale, b, x = _tensors(bits, K, N, M, 1)
    dt = x.dtype
    want = ref.fp8_ref(ref.as64(x), w8, ref.as64(scale), ref.as64(b))
    for cls, flag in ((ColumnParallelFp8Linear, False), (RowParallelFp8Linear, True)):
        lin = cls(K, N, True, flag, _pa(), dt, DEV)
        lin.load_state_dict({"weight": w8.cpu(), "weight_scale": scale.cpu()[:, None], "bias": b.cpu(),
                             "input_scale": torch.tensor(0.5)})         # a checkpoint arrives on the host
        lin.verify_loaded_weights()
        assert lin.weight.dtype == torch.float8_e4m3fn and lin.weight.is_cuda and torch.equal(lin.weight_scale, scale)
        y = lin.forward(x)
        assert y.shape == (M, N) and y.dtype == dt
        assert ref.rel_err(ref.as64(y), want) < ref.GEMM_TOL[bits], cls.__name__
    # a deferred call: the slabs' consumer sees what forward(out=...) would have written
    plain = RowParallelFp8Linear(K, N, False, True, _pa(), dt, DEV)
    plain.load_state_dict({"weight": w8, "weight_scale": scale})
    with kernels.tuning(SLM_LINEAR_SPLITK=2):
        written = plain.forward(x)
        assert plain.deferred_splits == 0 and not plain.deferred
        unwritten = plain.forward(x, defer_splitk=True)
        assert plain.deferred_splits == 2 and plain.deferred
        nw_ = torch.ones(N, dtype=dt, device=DEV)
        o1, o2 = torch.empty_like(written), torch.empty_like(written)
        kernels.rms_norm(o2, unwritten, nw_, 1e-5, partials=plain.deferred)
        kernels.rms_norm(o1, written, nw_, 1e-5)
        assert torch.equal(o1, o2)


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M", [1, 40])
def test_fused_gate_up_with_two_per_tensor_scales_equals_plain_then_silu_and_mul(M, bits):
    from scalellm_amd import kernels
    from scalellm_amd.layers import ColumnParallelFp8Linear
    K, N = 1024, 384
    g8, gs, _, x = _tensors(bits, K, N // 2, M, 4, per="tensor")
    u8, us, _, _ = _tensors(bits, K, N // 2, M, 5, per="tensor")
    us = us * 1.5                                                       # two DIFFERENT per-tensor scales
    assert float(gs[0]) != float(us[0])
    dt = x.dtype
    prefixes = ["gate_proj.", "up_proj."]
    gu = ColumnParallelFp8Linear(K, N, False, False, _pa(), dt, DEV, act_mul="silu")
    gu.load_state_dict({"up_proj.weight": u8, "up_proj.weight_scale": us[0]}, prefixes)
    gu.load_state_dict({"gate_proj.weight": g8, "gate_proj.weight_scale": gs[:1]}, prefixes)
    gu.verify_loaded_weights()
    assert torch.equal(gu.weight_scale, torch.cat([gs, us]))
    act = gu.forward(x)
    assert act.shape == (M, N // 2)
    w8 = torch.cat([g8.view(torch.uint8), u8.view(torch.uint8)]).view(torch.float8_e4m3fn)
    full = torch.empty(M, N, dtype=dt, device=DEV)
    unfused = torch.empty(M, N // 2, dtype=dt, device=DEV)
    with kernels.tuning(SLM_LINEAR_SPLITK=1):                           # the SiLU form never splits over K
        kernels.fp8_linear(x, w8, gu.weight_scale, full)
    kernels.silu_and_mul(unfused, full)
    assert torch.equal(act, unfused)
    y64 = ref.as64(ref.rounded(ref.fp8_ref(ref.as64(x), w8, ref.as64(gu.weight_scale)), bits))
    assert ref.rel_err(ref.as64(act), ref.silu_mul_ref(y64)) < ref.GEMM_TOL[bits]


@pytest.mark.parametrize("bits", ref.DTYPES)
def test_world_two_shards_run_in_turn(bits):
    from scalellm_amd.layers import ColumnParallelFp8Linear, RowParallelFp8Linear
    K, N, M = 512, 256, 33
    w8, scale, b, x = _tensors(bits, K, N, M, 2)
    dt = x.dtype
    sd = {"weight": w8, "weight_scale": scale, "bias": b}
    whole = ColumnParallelFp8Linear(K, N, True, False, _pa(), dt, DEV)
    whole.load_state_dict(sd)
    y = whole.forward(x)
    want = ref.fp8_ref(ref.as64(x), w8, ref.as64(scale), ref.as64(b))
    assert ref.rel_err(ref.as64(y), want) < ref.GEMM_TOL[bits]
    parts = []
    for rank in (0, 1):
        col = ColumnParallelFp8Linear(K, N, True, False, _pa(rank, 2), dt, DEV)     # gather_output=False
        col.load_state_dict(sd)
        col.verify_loaded_weights()
        parts.append(col.forward(x))
        assert parts[-1].shape == (M, N // 2)
    # a column depends on its own weight row and scale only, and K = 512 is too shallow for a K split at either width
    assert torch.equal(torch.cat(parts, dim=1), y)
    assert ref.rel_err(ref.as64(torch.cat(parts, dim=1)), want) < ref.GEMM_TOL[bits]
    total = torch.zeros(M, N, dtype=torch.float32, device=DEV)
    for rank in (0, 1):
        row = RowParallelFp8Linear(K, N, False, True, _pa(rank, 2), dt, DEV)       # input_is_parallelized
        row.load_state_dict({"weight": w8, "weight_scale": scale})
        assert torch.equal(row.weight_scale, scale)                                # whole on every rank
        total += row.forward(x[:, rank * (K // 2):(rank + 1) * (K // 2)].contiguous(), reduce=False).float()
    want = ref.fp8_ref(ref.as64(x), w8, ref.as64(scale))
    assert ref.rel_err(ref.as64(total), want) < ref.GEMM_TOL[bits]
    with_bias = RowParallelFp8Linear(K, N, True, True, _pa(0, 2), dt, DEV)
    with_bias.load_state_dict(sd)
    with pytest.raises(ValueError):
        with_bias.forward(x[:, :K // 2].contiguous(), reduce=False)    # the bias belongs after the reduction


@pytest.mark.parametrize("bits", ref.DTYPES)
def test_shim_classes_equal_the_python_classes_bit_for_bit(bits):
    from scalellm_amd import cpp_host, kernels
    from scalellm_amd.layers import ColumnParallelFp8Linear, RowParallelFp8Linear
    shim = cpp_host.load_shim()
    K, N = 1024, 256
    w8, scale, b, _ = _tensors(bits, K, N, 1, 3)
    dt = b.dtype
    q, k, v = w8[:128], w8[128:192], w8[192:]
    kv_scale = scale[128:192].mean()                                    # k: one per-tensor scale, 0-d
    file1 = {"q_proj.weight": q, "q_proj.weight_scale": scale[:128, None].double(), "v_proj.bias": b[192:],
             "k_proj.bias": b[128:192]}
    file2 = {"k_proj.weight": k, "k_proj.weight_scale": kv_scale, "v_proj.weight": v,
             "v_proj.weight_scale": scale[192:].to(torch.bfloat16), "q_proj.bias": b[:128],
             "k_proj.input_scale": torch.tensor(2.0)}
    prefixes = ["q_proj.", "k_proj.", "v_proj."]
    for M in (1, 33, 130):
        x = torch.randn(M, K, device=DEV, dtype=dt)
        for rank, world in ((0, 1), (1, 2)):
            py = ColumnParallelFp8Linear(K, N, True, False, _pa(rank, world), dt, DEV)
            cc = shim.create_column_parallel_fp8_linear(K, N, True, False, rank, world, dt, 0)
            for lin, fused in ((py, lambda s: py.load_state_dict(s, prefixes)),
                               (cc, lambda s: cc.load_state_dict_fused(s, prefixes))):
                fused(file2)
                with pytest.raises(RuntimeError, match="not loaded"):
                    lin.verify_loaded_weights()
                fused(file1)
                lin.verify_loaded_weights()
            with pytest.raises(RuntimeError, match="loaded twice"):
                cc.load_state_dict_fused(file1, prefixes)
            assert torch.equal(cc.forward(x), py.forward(x)), (M, rank, world)
            pr = RowParallelFp8Linear(K, N, world == 1, True, _pa(rank, world), dt, DEV)
            cr = shim.create_row_parallel_fp8_linear(K, N, world == 1, True, rank, world, dt, 0)
            pr.load_state_dict({"weight": w8, "weight_scale": scale, "bias": b})
            cr.load_state_dict({"weight": w8, "weight_scale": scale, "bias": b})
            xr = x[:, rank * (K // world):(rank + 1) * (K // world)].contiguous()
            assert torch.equal(cr.forward(xr), pr.forward(xr, reduce=world == 1)), (M, rank, world)
        pg = ColumnParallelFp8Linear(K, N, False, False, _pa(), dt, DEV, act_mul="silu")
        cg = shim.create_column_parallel_fp8_linear(K, N, False, False, 0, 1, dt, 0, act_mul_silu=True)
        pg.load_state_dict({"weight": w8, "weight_scale": scale})
        cg.load_state_dict({"weight": w8, "weight_scale": scale})
        assert torch.equal(cg.forward(x), pg.forward(x))
        direct = torch.empty(M, N, dtype=dt, device=DEV)
        kernels.fp8_linear(x, w8, scale, direct, b)
        assert torch.equal(shim.fp8_linear(x, w8, scale, b), direct)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        cc = shim.create_column_parallel_fp8_linear(K, N, False, False, 0, 1, dt, 0)
        cc.load_state_dict({"weight": w8.to(dt), "weight_scale": scale})
    with pytest.raises(RuntimeError, match="fp16 / bf16"):
        shim.create_row_parallel_fp8_linear(256, 256, False, True, 0, 1, torch.float32, 0)
