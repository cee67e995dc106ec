"""The MXFP4 weight-only linear LAYERS (layers.ColumnParallelMxfp4Linear / RowParallelMxfp4Linear and their C++ twins
slm::{Column,Row}ParallelMxfp4LinearHipImpl) on the GPU: bit for bit against kernels.mxfp4_linear on their own
weights and within the GEMM tolerance of float64 over the same quantised weights, the fused gate | up load against
the plain call + silu_and_mul, a two-way row shard summed on the one GPU, and the shim classes against the Python
classes."""
import pytest
import torch

from . import mxfp4_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pa(rank=0, world=1):
    from scalellm_amd.model_parallel import ParallelArgs
    return ParallelArgs(rank=rank, world_size=world)


def _tensors(bits, K, N, M, seed):
    from scalellm_amd import kernels
    g = torch.Generator(device=DEV).manual_seed(seed)
    dt = ref.torch_dtype(bits)
    w, sc = kernels.quantize_mxfp4_weight(torch.randn(N, K, device=DEV, generator=g) * 0.05)
    b = torch.randn(N, device=DEV, generator=g).to(dt)
    x = torch.randn(M, K, device=DEV, generator=g).to(dt)
    return w, sc, b, x


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M", [1, 40])
def test_python_layers_equal_the_kernel_call_on_their_own_weights(M, bits):
    from scalellm_amd import kernels
    from scalellm_amd.layers import ColumnParallelMxfp4Linear, RowParallelMxfp4Linear
    K, N = 1024, 384
    w, sc, b, x = _tensors(bits, K, N, M, 1)
    dt = x.dtype
    want = ref.mxfp4_ref(ref.as64(x), w, sc, ref.as64(b))
    direct = torch.empty(M, N, dtype=dt, device=DEV)
    kernels.mxfp4_linear(x, w, sc, direct, b)
    forms = [(w.cpu(), sc.cpu()), (w.cpu().view(N, K // 32, 16), sc.cpu())]     # a checkpoint arrives on the host
    if hasattr(torch, "float4_e2m1fn_x2") and hasattr(torch, "float8_e8m0fnu"):
        forms.append((w.cpu().view(torch.float4_e2m1fn_x2), sc.cpu().view(torch.float8_e8m0fnu)))
    for cls, flag in ((ColumnParallelMxfp4Linear, False), (RowParallelMxfp4Linear, True)):
        for wf, sf in forms:
            lin = cls(K, N, True, flag, _pa(), dt, DEV)
            lin.load_state_dict({"weight": wf, "weight_scale": sf, "bias": b.cpu()})
            lin.verify_loaded_weights()
            assert lin.weight.dtype == torch.uint8 and lin.weight.is_cuda and torch.equal(lin.weight, w)
            assert torch.equal(lin.weight_scale, sc)
            y = lin.forward(x)
            assert y.shape == (M, N) and y.dtype == dt
            assert torch.equal(y, direct), cls.__name__
        assert ref.rel_err(ref.as64(y), want) < ref.GEMM_TOL[bits], cls.__name__
    # a deferred call: the slabs' consumer sees what forward(out=...) would have written
    plain = RowParallelMxfp4Linear(K, N, False, True, _pa(), dt, DEV)
    plain.load_state_dict({"weight": w, "weight_scale": sc})
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
def test_fused_gate_up_equals_plain_then_silu_and_mul(M, bits):
    from scalellm_amd import kernels
    from scalellm_amd.layers import ColumnParallelMxfp4Linear
    K, N = 1024, 384
    gw, gs, _, x = _tensors(bits, K, N // 2, M, 4)
    uw, us, _, _ = _tensors(bits, K, N // 2, M, 5)
    dt = x.dtype
    prefixes = ["gate_proj.", "up_proj."]
    gu = ColumnParallelMxfp4Linear(K, N, False, False, _pa(), dt, DEV, act_mul="silu")
    gu.load_state_dict({"up_proj.weight": uw, "up_proj.weight_scale": us}, prefixes)
    gu.load_state_dict({"gate_proj.weight": gw, "gate_proj.weight_scale": gs}, prefixes)
    gu.verify_loaded_weights()
    w, sc = torch.cat([gw, uw]), torch.cat([gs, us])
    assert torch.equal(gu.weight, w) and torch.equal(gu.weight_scale, sc)
    act = gu.forward(x)
    assert act.shape == (M, N // 2)
    fused = torch.empty(M, N // 2, dtype=dt, device=DEV)
    kernels.mxfp4_linear(x, w, sc, fused, silu_mul=True)
    assert torch.equal(act, fused)
    full = torch.empty(M, N, dtype=dt, device=DEV)
    unfused = torch.empty(M, N // 2, dtype=dt, device=DEV)
    with kernels.tuning(SLM_LINEAR_SPLITK=1):                           # the SiLU form never splits over K
        kernels.mxfp4_linear(x, w, sc, full)
    kernels.silu_and_mul(unfused, full)
    assert torch.equal(act, unfused)
    y64 = ref.as64(ref.rounded(ref.mxfp4_ref(ref.as64(x), w, sc), bits))
    assert ref.rel_err(ref.as64(act), ref.silu_mul_ref(y64)) < ref.GEMM_TOL[bits]


@pytest.mark.parametrize("bits", ref.DTYPES)
def test_world_two_shards_run_in_turn(bits):
    from scalellm_amd import kernels
    from scalellm_amd.layers import ColumnParallelMxfp4Linear, RowParallelMxfp4Linear
    K, N, M = 512, 256, 33
    w, sc, b, x = _tensors(bits, K, N, M, 2)
    dt = x.dtype
    sd = {"weight": w, "weight_scale": sc, "bias": b}
    whole = ColumnParallelMxfp4Linear(K, N, True, False, _pa(), dt, DEV)
    whole.load_state_dict(sd)
    y = whole.forward(x)
    want = ref.mxfp4_ref(ref.as64(x), w, sc, ref.as64(b))
    assert ref.rel_err(ref.as64(y), want) < ref.GEMM_TOL[bits]
    parts = []
    for rank in (0, 1):
        col = ColumnParallelMxfp4Linear(K, N, True, False, _pa(rank, 2), dt, DEV)     # gather_output=False
        col.load_state_dict(sd)
        col.verify_loaded_weights()
        parts.append(col.forward(x))
        assert parts[-1].shape == (M, N // 2)
    # a column depends on its own weight and scale rows only, and K = 512 is too shallow for a K split at either width
    assert torch.equal(torch.cat(parts, dim=1), y)
    total = torch.zeros(M, N, dtype=torch.float32, device=DEV)
    for rank in (0, 1):
        row = RowParallelMxfp4Linear(K, N, False, True, _pa(rank, 2), dt, DEV)       # input_is_parallelized
        row.load_state_dict({"weight": w, "weight_scale": sc})
        assert torch.equal(row.weight, w[:, rank * (K // 4):(rank + 1) * (K // 4)])
        assert torch.equal(row.weight_scale, sc[:, rank * (K // 64):(rank + 1) * (K // 64)])
        xr = x[:, rank * (K // 2):(rank + 1) * (K // 2)].contiguous()
        part = row.forward(xr, reduce=False)
        direct = torch.empty(M, N, dtype=dt, device=DEV)
        kernels.mxfp4_linear(xr, row.weight, row.weight_scale, direct)
        assert torch.equal(part, direct)
        total += part.float()
    want = ref.mxfp4_ref(ref.as64(x), w, sc)
    assert ref.rel_err(ref.as64(total), want) < ref.GEMM_TOL[bits]
    with_bias = RowParallelMxfp4Linear(K, N, True, True, _pa(0, 2), dt, DEV)
    with_bias.load_state_dict(sd)
    with pytest.raises(ValueError):
        with_bias.forward(x[:, :K // 2].contiguous(), reduce=False)    # the bias belongs after the reduction


@pytest.mark.parametrize("bits", ref.DTYPES)
def test_shim_classes_equal_the_python_classes_bit_for_bit(bits):
    from scalellm_amd import cpp_host, kernels
    from scalellm_amd.layers import ColumnParallelMxfp4Linear, RowParallelMxfp4Linear
    shim = cpp_host.load_shim()
    K, N = 1024, 256
    w, sc, b, _ = _tensors(bits, K, N, 1, 3)
    dt = b.dtype
    file1 = {"q_proj.weight": w[:128], "q_proj.weight_scale": sc[:128], "v_proj.bias": b[192:], "k_proj.bias": b[128:192]}
    file2 = {"k_proj.weight": w[128:192].view(64, K // 32, 16), "k_proj.weight_scale": sc[128:192],
             "v_proj.weight": w[192:], "v_proj.weight_scale": sc[192:], "q_proj.bias": b[:128]}
    prefixes = ["q_proj.", "k_proj.", "v_proj."]
    M = 33
    x = torch.randn(M, K, device=DEV, dtype=dt)
    for rank, world in ((0, 1), (1, 2)):
        py = ColumnParallelMxfp4Linear(K, N, True, False, _pa(rank, world), dt, DEV)
        cc = shim.create_column_parallel_mxfp4_linear(K, N, True, False, rank, world, dt, 0)
        for lin, fused in ((py, lambda s: py.load_state_dict(s, prefixes)),
                           (cc, lambda s: cc.load_state_dict_fused(s, prefixes))):
            fused(file2)
            with pytest.raises(RuntimeError, match="not loaded"):
                lin.verify_loaded_weights()
            fused(file1)
            lin.verify_loaded_weights()
        with pytest.raises(RuntimeError, match="loaded twice"):
            cc.load_state_dict_fused(file1, prefixes)
        assert torch.equal(cc.forward(x), py.forward(x)), (rank, world)
        pr = RowParallelMxfp4Linear(K, N, world == 1, True, _pa(rank, world), dt, DEV)
        cr = shim.create_row_parallel_mxfp4_linear(K, N, world == 1, True, rank, world, dt, 0)
        pr.load_state_dict({"weight": w, "weight_scale": sc, "bias": b})
        cr.load_state_dict({"weight": w, "weight_scale": sc, "bias": b})
        xr = x[:, rank * (K // world):(rank + 1) * (K // world)].contiguous()
        assert torch.equal(cr.forward(xr), pr.forward(xr, reduce=world == 1)), (rank, world)
    pg = ColumnParallelMxfp4Linear(K, N, False, False, _pa(), dt, DEV, act_mul="silu")
    cg = shim.create_column_parallel_mxfp4_linear(K, N, False, False, 0, 1, dt, 0, act_mul_silu=True)
    pg.load_state_dict({"weight": w, "weight_scale": sc})
    cg.load_state_dict({"weight": w, "weight_scale": sc})
    assert torch.equal(cg.forward(x), pg.forward(x))
    direct = torch.empty(M, N, dtype=dt, device=DEV)
    kernels.mxfp4_linear(x, w, sc, direct, b)
    assert torch.equal(shim.mxfp4_linear(x, w, sc, b), direct)
    with pytest.raises(RuntimeError, match="uint8"):
        cc = shim.create_column_parallel_mxfp4_linear(K, N, False, False, 0, 1, dt, 0)
        cc.load_state_dict({"weight": torch.zeros(N, K, dtype=dt, device=DEV), "weight_scale": sc})
    with pytest.raises(RuntimeError, match="fp16 / bf16"):
        shim.create_row_parallel_mxfp4_linear(256, 256, False, True, 0, 1, torch.float32, 0)
