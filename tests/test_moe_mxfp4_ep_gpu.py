"""ExpertParallelMoE over OCP MXFP4 experts: two ranks on one GPU with their own worker, the arrangement of
tests/test_moe_fp8_ep_gpu.py (gloo collectives staged through host tensors; that file's staging group lives inside its
worker function, so it is restated here and only the free-port helper is imported).  Every rank's output is compared
with a one-rank FusedMoE over the same checkpoint: the same nibbles and scale bytes, the expert shards found through
expert_offset.  The two layers round at other points (the rows travel in T and the routing weight is applied after the
down GEMM's rounding), which is the 2 x GEMM_TOL tests/test_token_dispatcher_gpu.py allows its ExpertParallelMoE; the
rank's stacked nibble and scale bytes are compared bit for bit with its slice of the one-rank layer's."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from .moe_dense_ref import GEMM_TOL, rel_err
from .moe_mxfp4_ref import MOE_LAYER, MOE_TOKENS, as64, mxfp4_state_dict, torch_dtype
from .test_token_dispatcher_gpu import _free_port

pytestmark = pytest.mark.gpu

HID, INTER, NE, TOPK = (MOE_LAYER[k] for k in ("hidden", "intermediate", "n_experts", "topk"))


def _worker(rank, world, port, q):
    try:
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                          LOCAL_RANK="0", SLM_DIST_BACKEND="gloo")
        from scalellm_amd import moe
        from scalellm_amd.layers import QuantArgs
        from scalellm_amd.model_parallel import ProcessGroup

        class HostStagedGroup(ProcessGroup):
            """gloo runs these two collectives on host tensors; the product class hands over device tensors"""

            def allgather_into(self, tensor, output):
                host = torch.empty(output.shape, dtype=output.dtype)
                super().allgather_into(tensor.cpu(), host)
                output.copy_(host)

            def alltoall(self, tensor, output, input_split_sizes=None, output_split_sizes=None):
                host = torch.empty(output.shape, dtype=output.dtype).view(torch.uint8)
                super().alltoall(tensor.cpu().contiguous().view(torch.uint8), host, input_split_sizes,
                                 output_split_sizes)
                output.copy_(host.view(output.dtype))

        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        ProcessGroup.create_from_env(dev)
        pg = HostStagedGroup()
        assert (pg.rank, pg.world_size) == (rank, world)
        res = {"rank": rank}
        q4 = QuantArgs("mxfp4", 4)
        L = NE // world
        for bits in ("bf16", "f16"):
            sd, dt = mxfp4_state_dict(HID, INTER, NE, bits), torch_dtype(bits)
            ep = moe.ExpertParallelMoE(HID, INTER, NE, TOPK, pg, q4, dtype=dt, device=dev)
            ep.load_state_dict(sd)
            local = moe.FusedMoE(HID, INTER, NE, TOPK, q4, max_tokens=max(MOE_TOKENS), dtype=dt, device=dev)
            local.load_state_dict(sd)
            assert isinstance(ep.experts, moe.MoEMxfp4Experts)
            assert (ep.experts.n_experts, ep.experts.expert_offset) == (L, rank * L)
            g = torch.Generator(device=dev).manual_seed(11 + rank)
            for T in MOE_TOKENS:                                               # both ranks: the same count of calls
                x = torch.randn(T, HID, device=dev, dtype=dt, generator=g)
                y = ep(x)
                assert y.shape == x.shape and not bool(torch.isnan(y).any())
                res[f"err_{bits}_{T}"] = rel_err(as64(y), as64(local(x)))
                assert torch.equal(ep(x), y)                                   # bit-identical repeats
            for name in ("gate_up", "gate_up_scale", "down", "down_scale"):    # this rank's shard of the stacked bytes
                assert torch.equal(getattr(ep.experts, name), getattr(local.experts, name)[rank * L:(rank + 1) * L])
        pg.barrier()
        torch.distributed.destroy_process_group()
        q.put(res)
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put({"rank": rank, "fail": repr(e) + traceback.format_exc()})


@pytest.mark.timeout(300)
def test_mxfp4_experts_on_two_ranks_match_one_rank():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    assert all("fail" not in r for r in res), res
    for r in res:
        for bits in ("bf16", "f16"):
            for T in MOE_TOKENS:
                print(f"[ep mxfp4 moe] rank {r['rank']} {bits} T={T}: rel err {r[f'err_{bits}_{T}']:.2e}")
                assert r[f"err_{bits}_{T}"] < 2 * GEMM_TOL[bits], r         # two chained GEMMs, GEMM_TOL each
