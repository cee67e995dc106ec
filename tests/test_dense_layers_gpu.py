"""The unquantised linear LAYERS (layers.ColumnParallelLinear / RowParallelLinear and their C++ twins
slm::{Column,Row}ParallelLinearHipImpl) on the GPU: against x @ W.T + b in float64, tensor-parallel shards of one
layer run in turn on the one GPU, and the shim classes bit for bit against the Python classes."""
import numpy as np
import pytest
import torch

from . import dense_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pa(rank=0, world=1):
    from scalellm_amd.model_parallel import ParallelArgs
    return ParallelArgs(rank=rank, world_size=world)


def _tensors(bits, K, N, M, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    dt = ref.torch_dtype(bits)
    w = (torch.randn(N, K, device=DEV, generator=g) * 0.05).to(dt)
    b = torch.randn(N, device=DEV, generator=g).to(dt)
    x = torch.randn(M, K, device=DEV, generator=g).to(dt)
    return w, b, x


@pytest.mark.parametrize("bits", ref.DTYPES)
@pytest.mark.parametrize("M", [1, 40])
def test_python_layers_against_float64(M, bits):
    from scalellm_amd.layers import ColumnParallelLinear, RowParallelLinear
    K, N = 1024, 384
    w, b, x = _tensors(bits, K, N, M, 1)
    want = ref.linear_ref(ref.as64(x), ref.as64(w), ref.as64(b))
    for cls, flag in ((ColumnParallelLinear, False), (RowParallelLinear, True)):
        lin = cls(K, N, True, flag, _pa(), w.dtype, DEV)
        lin.load_state_dict({"weight": w.cpu(), "bias": b.cpu()})       # a checkpoint arrives on the host
        lin.verify_loaded_weights()
        y = lin.forward(x)
        assert y.shape == (M, N) and y.dtype == w.dtype
        assert ref.rel_err(ref.as64(y), want) < ref.GEMM_TOL[bits], cls.__name__
    # the merged gate | up projection with the fused activation, loaded from its two prefixes
    gu = ColumnParallelLinear(K, N, False, False, _pa(), w.dtype, DEV, act_mul="silu")
    gu.load_state_dict({"up_proj.weight": w[N // 2:]}, ["gate_proj.", "up_proj."])
    gu.load_state_dict({"gate_proj.weight": w[:N // 2]}, ["gate_proj.", "up_proj."])
    act = gu.forward(x)
    y64 = ref.as64(ref.rounded(ref.linear_ref(ref.as64(x), ref.as64(w)), bits))
    assert act.shape == (M, N // 2)
    assert ref.rel_err(ref.as64(act), ref.silu_mul_ref(y64)) < ref.GEMM_TOL[bits]
    # a deferred call: the slabs' consumer sees what forward(out=...) would have written
    from scalellm_amd import kernels
    plain = RowParallelLinear(K, N, False, True, _pa(), w.dtype, DEV)
    plain.load_state_dict({"weight": w})
    with kernels.tuning(SLM_LINEAR_SPLITK=2):
        written = plain.forward(x)
        assert plain.deferred_splits == 0 and not plain.deferred
        unwritten = plain.forward(x, defer_splitk=True)
        assert plain.deferred_splits == 2 and plain.deferred
        nw_ = torch.ones(N, dtype=w.dtype, device=DEV)
        o1, o2 = torch.empty_like(written), torch.empty_like(written)
        kernels.rms_norm(o2, unwritten, nw_, 1e-5, partials=plain.deferred)
        kernels.rms_norm(o1, written, nw_, 1e-5)
        assert torch.equal(o1, o2)


@pytest.mark.parametrize("bits", ref.DTYPES)
def test_world_two_shards_run_in_turn(bits):
    from scalellm_amd.layers import ColumnParallelLinear, RowParallelLinear
    K, N, M = 512, 256, 33
    w, b, x = _tensors(bits, K, N, M, 2)
    sd = {"weight": w, "bias": b}
    whole = ColumnParallelLinear(K, N, True, False, _pa(), w.dtype, DEV)
    whole.load_state_dict(sd)
    y = whole.forward(x)
    parts = []
    for rank in (0, 1):
        col = ColumnParallelLinear(K, N, True, False, _pa(rank, 2), w.dtype, DEV)   # gather_output=False
        col.load_state_dict(sd)
        col.verify_loaded_weights()
        parts.append(col.forward(x))
        assert parts[-1].shape == (M, N // 2)
    # a column of the output depends on its own weight row only, and an element's accumulation order does not depend
    # on the row tiles or waves of the launch (K = 512 is too shallow for a K split at either width): the shards are
    # the unsharded layer's columns
    assert torch.equal(torch.cat(parts, dim=1), y)
    total = torch.zeros(M, N, dtype=torch.float32, device=DEV)
    for rank in (0, 1):
        row = RowParallelLinear(K, N, False, True, _pa(rank, 2), w.dtype, DEV)     # input_is_parallelized
        row.load_state_dict({"weight": w})
        total += row.forward(x[:, rank * (K // 2):(rank + 1) * (K // 2)].contiguous(), reduce=False).float()
    want = ref.linear_ref(ref.as64(x), ref.as64(w))
    assert ref.rel_err(ref.as64(total), want) < ref.GEMM_TOL[bits]
    with_bias = RowParallelLinear(K, N, True, True, _pa(0, 2), w.dtype, DEV)
    with_bias.load_state_dict(sd)
    with pytest.raises(ValueError):
        with_bias.forward(x[:, :K // 2].contiguous(), reduce=False)    # the bias belongs after the reduction


@pytest.mark.parametrize("bits", ref.DTYPES)
def test_shim_classes_equal_the_python_classes_bit_for_bit(bits):
    from scalellm_amd import cpp_host
    from scalellm_amd.layers import ColumnParallelLinear, RowParallelLinear
    shim = cpp_host.load_shim()
    K, N = 1024, 256
    w, b, _ = _tensors(bits, K, N, 1, 3)
    dt = w.dtype
    q, k, v = w[:128], w[128:192], w[192:]
    file1 = {"q_proj.weight": q, "v_proj.bias": b[192:], "k_proj.bias": b[128:192]}
    file2 = {"k_proj.weight": k, "v_proj.weight": v, "q_proj.bias": b[:128]}
    prefixes = ["q_proj.", "k_proj.", "v_proj."]
    for M in (1, 33, 130):
        x = torch.randn(M, K, device=DEV, dtype=dt)
        for rank, world in ((0, 1), (1, 2)):
            py = ColumnParallelLinear(K, N, True, False, _pa(rank, world), dt, DEV)
            cc = shim.create_column_parallel_linear(K, N, True, False, "", rank, world, dt, 0)
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
            pr = RowParallelLinear(K, N, world == 1, True, _pa(rank, world), dt, DEV)
            cr = shim.create_row_parallel_linear(K, N, world == 1, True, "", rank, world, dt, 0)
            pr.load_state_dict({"weight": w, "bias": b})
            cr.load_state_dict({"weight": w, "bias": b})
            xr = x[:, rank * (K // world):(rank + 1) * (K // world)].contiguous()
            assert torch.equal(cr.forward(xr), pr.forward(xr, reduce=world == 1)), (M, rank, world)
        # the merged gate | up projection with the SiLU epilogue
        pg = ColumnParallelLinear(K, N, False, False, _pa(), dt, DEV, act_mul="silu")
        cg = shim.create_column_parallel_linear(K, N, False, False, "", 0, 1, dt, 0, act_mul_silu=True)
        pg.load_state_dict({"weight": w})
        cg.load_state_dict({"weight": w})
        assert torch.equal(cg.forward(x), pg.forward(x))


def test_factories_keep_refusing_unknown_quant_methods():
    from scalellm_amd import cpp_host
    shim = cpp_host.load_shim()
    with pytest.raises(RuntimeError, match="Unsupported quant method"):
        shim.create_column_parallel_qlinear(256, 256, False, False, "squeezellm", 4, 128, False, False, True, 0, 1,
                                            torch.bfloat16, 0)
    with pytest.raises(RuntimeError, match="Unsupported quant method"):
        shim.create_row_parallel_qlinear(256, 256, False, True, "squeezellm", 4, 128, False, False, True, 0, 1,
                                         torch.bfloat16, 0)
    # ... and the dense factory hands a named method on to them
    with pytest.raises(RuntimeError, match="Unsupported quant method"):
        shim.create_column_parallel_linear(256, 256, False, False, "squeezellm", 0, 1, torch.bfloat16, 0)
    q = shim.create_column_parallel_linear(256, 256, False, False, "awq", 0, 1, torch.bfloat16, 0)
    with pytest.raises(RuntimeError, match="qweight is not loaded"):
        q.verify_loaded_weights()
    with pytest.raises(RuntimeError, match="fp16 / bf16"):
        shim.create_row_parallel_linear(256, 256, False, True, "", 0, 1, torch.float32, 0)
    with pytest.raises(RuntimeError, match="not divisible"):
        shim.create_row_parallel_linear(250, 256, False, True, "", 0, 4, torch.bfloat16, 0)
