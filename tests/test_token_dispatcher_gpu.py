"""GPU tests of the token dispatchers (scalellm_amd/moe.py): the reference's round-trip grid (token_dispatcher_test.cpp:
127-136) for LocalTokenDispatcher and for AlltoAllTokenDispatcher at world size 1, through both entry points; graph
replay of the local dispatcher; and one two-rank run on ONE GPU over gloo (RCCL needs one GPU per rank) that checks the
round trip, every rank's received rows against the numpy simulator, and ExpertParallelMoE against the float64
composition."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from . import moe_ref
from . import permute_ref as ref
from .moe_dense_ref import GEMM_TOL, as64, rel_err, rounded, torch_dtype

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIM, MAX_TOKENS = 32, 16


def _routing(rng, T, E, k, bits):
    """the reference test's inputs: top-k of random logits, probs = 1 / k on the routed experts"""
    dt = torch_dtype(bits)
    ids = ref.distinct_ids(rng, T, k, E)
    mask = torch.from_numpy(ref.ids_to_mask(ids, E)).to(DEV)
    probs = (mask.float() / k).to(dt)
    weights = torch.full((T, k), 1.0 / k, device=DEV)
    x = rounded(rng.standard_normal((T, DIM)), bits).to(DEV)
    return x, ids, mask, probs, weights


def _dispatchers(E, k):
    from scalellm_amd import moe
    from scalellm_amd.model_parallel import ProcessGroup
    return [("local", moe.LocalTokenDispatcher(k, E)), ("alltoall", moe.AlltoAllTokenDispatcher(E, k, ProcessGroup()))]


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("E", [8, 64])
@pytest.mark.parametrize("bits", ["f16", "bf16"])
def test_round_trip_grid(bits, E, k):
    rng = np.random.default_rng(E + k)
    for T in (1, int(rng.integers(2, MAX_TOKENS)), MAX_TOKENS):
        x, ids, mask, probs, weights = _routing(rng, T, E, k, bits)
        want_rows = ref.permute_rows(as64(x), ref.index_map(ids, E)[0], np.zeros((T * k, DIM)))
        bincount = np.bincount(ids.reshape(-1), minlength=E)
        for name, d in _dispatchers(E, k):
            for entry in ("mask", "topk"):
                if entry == "mask":
                    permuted, counts = d.dispatch(x, probs, mask)
                else:
                    permuted, counts = d.dispatch_topk(x, weights, torch.from_numpy(ids).to(DEV))
                what = (name, entry, T)
                assert permuted.shape == (T * k, DIM) and counts.shape == (E,), what
                assert np.array_equal(counts.cpu().numpy(), bincount), what
                assert np.array_equal(as64(permuted), want_rows), what       # distinct ids: both forms, one order
                out = d.combine(permuted, None)
                assert torch.equal(out, x), what                             # k * (1 / k) with k in {1, 4}: exact


def test_local_dispatcher_graph_replay_over_a_changed_routing():
    from scalellm_amd import moe
    T, E, k = 5, 8, 2
    rng = np.random.default_rng(7)
    d = moe.LocalTokenDispatcher(k, E)
    x, ids, _, _, weights = _routing(rng, T, E, k, "bf16")
    ids_s = torch.from_numpy(ids).to(DEV)
    d.combine(d.dispatch_topk(x, weights, ids_s)[0])                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        permuted, counts = d.dispatch_topk(x, weights, ids_s)
        out = d.combine(permuted * 2)                                     # "experts": double every row
    for _ in range(3):
        ids = ref.distinct_ids(rng, T, k, E)
        ids_s.copy_(torch.from_numpy(ids))
        graph.replay()
        assert np.array_equal(counts.cpu().numpy(), np.bincount(ids.reshape(-1), minlength=E))
        want_rows = ref.permute_rows(as64(x), ref.index_map(ids, E)[0], np.zeros((T * k, DIM)))
        assert np.array_equal(as64(permuted), want_rows)
        assert torch.equal(out, x * 2)
    torch.cuda.synchronize()


# ---- world size 2 on one GPU ------------------------------------------------------------------------------------------
HID, INTER, NE, TOPK = 256, 384, 8, 2      # tests/test_moe_dense_gpu.py's sizes


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_inputs(rank, T, E, k, bits, seed):
    rng = np.random.default_rng(1000 * seed + rank)
    return rounded(rng.standard_normal((T, DIM)), bits), ref.distinct_ids(rng, T, k, E)


def _checkpoint(bits):
    dt = torch_dtype(bits)
    g = torch.Generator().manual_seed(0)
    sd = {}
    for e in range(NE):
        sd[f"experts.{e}.w1.weight"] = (torch.randn(INTER, HID, generator=g) / 16).to(dt)
        sd[f"experts.{e}.w3.weight"] = (torch.randn(INTER, HID, generator=g) / 16).to(dt)
        sd[f"experts.{e}.w2.weight"] = (torch.randn(HID, INTER, generator=g) / 16).to(dt)
    sd["gate.weight"] = (torch.randn(NE, HID, generator=g) * 0.5).to(dt)
    return sd


def _ep_moe_reference(sd, x, bits):
    """_moe_reference of tests/test_moe_dense_gpu.py with THIS path's rounding points: after SiLU * mul (of the rounded
    gate and up), after the down GEMM (the rows travel in the dtype), after the weighted sum"""
    rnd = lambda v: as64(rounded(v, bits))  # noqa: E731
    dense = {key: as64(v) for key, v in sd.items() if key.startswith("experts.")}
    logits = (x.float() @ sd["gate.weight"].to(x.device).float().t()).cpu().numpy()
    w, ids = moe_ref.topk_softmax(logits, TOPK, renormalize=True)
    x64 = as64(x)
    out = np.zeros((x.size(0), HID))
    for t in range(x.size(0)):
        terms = {}
        for j in range(TOPK):
            e = int(ids[t, j])
            gate = rnd(dense[f"experts.{e}.w1.weight"] @ x64[t])
            up = rnd(dense[f"experts.{e}.w3.weight"] @ x64[t])
            act = rnd(gate / (1 + np.exp(-gate)) * up)
            terms[e] = np.float32(w[t, j]).astype(np.float64) * rnd(dense[f"experts.{e}.w2.weight"] @ act)
        for e in sorted(terms):                                        # ascending expert order
            out[t] += terms[e]
    return rnd(out)


def _worker(rank, world, port, q):
    try:
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                          LOCAL_RANK="0", SLM_DIST_BACKEND="gloo")
        from scalellm_amd import moe
        from scalellm_amd.model_parallel import ProcessGroup

        class HostStagedGroup(ProcessGroup):
            """gloo runs these two collectives on host tensors (that is how they are exercised without a GPU); the
            product class hands over device tensors, as RCCL wants them, so this test's group stages them"""

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
        res = {"rank": rank, "cases": 0}
        # round trip + the rows every rank's experts see, against the simulator
        for seed, (bits, E, k) in enumerate((("bf16", 8, 1), ("f16", 8, 4), ("bf16", 64, 4), ("f16", 64, 1))):
            n_tok = [5 + seed, 16 - 3 * seed]                                  # uneven over the ranks
            data = [_rank_inputs(r, n_tok[r], E, k, bits, seed) for r in range(world)]
            sim_rows, sim_counts, sim_out = ref.simulate(world, E, [i for _, i in data], [as64(x) for x, _ in data],
                                                         [np.full((n, k), 1.0 / k) for n in n_tok])
            x, ids = data[rank]
            x = x.to(dev)
            assert np.array_equal(sim_out[rank], as64(x))
            d = moe.AlltoAllTokenDispatcher(E, k, pg)
            mask = torch.from_numpy(ref.ids_to_mask(ids, E)).to(dev)
            for entry in ("mask", "topk"):
                if entry == "mask":
                    rows, counts = d.dispatch(x, (mask.float() / k).to(x.dtype), mask)
                else:
                    rows, counts = d.dispatch_topk(x, torch.full((n_tok[rank], k), 1.0 / k, device=dev),
                                                   torch.from_numpy(ids).to(dev))
                assert np.array_equal(as64(rows), sim_rows[rank]), (entry, bits, E, k)
                assert np.array_equal(counts.cpu().numpy(), sim_counts[rank]), (entry, bits, E, k)
                assert torch.equal(d.combine(rows), x), (entry, bits, E, k)
                res["cases"] += 1
        # ExpertParallelMoE against the float64 composition over ALL experts
        for bits in ("bf16", "f16"):
            sd = _checkpoint(bits)
            layer = moe.ExpertParallelMoE(HID, INTER, NE, TOPK, pg, dtype=torch_dtype(bits), device=dev)
            layer.load_state_dict(sd)
            g = torch.Generator(device=dev).manual_seed(11 + rank)
            for T in (1, 5, 70):
                x = torch.randn(T, HID, device=dev, dtype=torch_dtype(bits), generator=g)
                y = layer(x)
                assert y.shape == x.shape and not bool(torch.isnan(y).any())
                err = rel_err(as64(y), _ep_moe_reference(sd, x, bits))
                res[f"moe_err_{bits}_{T}"] = err
                assert torch.equal(layer(x), y)                                # bit-identical repeats
        pg.barrier()
        torch.distributed.destroy_process_group()
        q.put(res)
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put({"rank": rank, "fail": repr(e) + traceback.format_exc()})


@pytest.mark.timeout(300)
def test_two_ranks_on_one_gpu():
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
        assert r["cases"] == 8, r
        for bits in ("bf16", "f16"):
            for T in (1, 5, 70):
                print(f"[ep moe] rank {r['rank']} {bits} T={T}: rel err {r[f'moe_err_{bits}_{T}']:.2e}")
                assert r[f"moe_err_{bits}_{T}"] < 2 * GEMM_TOL[bits], r      # two chained GEMMs, GEMM_TOL each
