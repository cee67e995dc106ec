"""bench.py's N > 1 path executed for real before the driver's first multi-GPU contact (VERDICT r1
item 2): `python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2 ...` exactly as the
driver launches it, with both ranks on the ONE GPU of this box (SLM_FORCE_LOCAL_RANK=0) and gloo
standing in for RCCL (RCCL needs one GPU per rank).  Everything else is the production path:
torchrun rendezvous on 127.0.0.1, one process per rank, TP sharding of heads / N / K, the
row-parallel reductions (fused xGMI kernel over real interprocess mappings, or the collective
fallback), barrier + MAX-over-ranks timing, rank 0 printing ONE JSON line.

Checks: one JSON line; n_gpus == 2; the reduce path and the collective census are reported; the two
row-parallel-reduce paths (fused kernel vs collective + slm_rms_norm) produce IDENTICAL first-step
tokens (both sum in fp32 in rank order); and those agree with the single-rank run of the same
model on >= 75 % of the rows (TP changes the fp32 summation order inside every row-parallel GEMM,
so a near-tie may flip: test_tp_gpu.py bounds the logits themselves).
"""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--layers", "2", "--bs", "8", "--seqlen", "256", "--steps", "2", "--warmup", "1",
          "--no-cpu-baseline", "--no-traffic", "--kv-fill", "consistent"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(cmd, env_extra):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", GPU_MAX_HW_QUEUES="8", **env_extra)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=560)
    assert r.returncode == 0, f"{' '.join(cmd)}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"expected ONE JSON line, got {len(lines)}:\n{r.stdout[-2000:]}"
    return json.loads(lines[0]), r.stderr


def _torchrun(n, extra_env, model_args=()):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py",
           "--gpus", str(n), *COMMON, *model_args]
    return _run(cmd, dict(SLM_FORCE_LOCAL_RANK="0", SLM_DIST_BACKEND="gloo", **extra_env))


@pytest.mark.timeout(1800)
def test_bench_two_ranks_one_gpu_json_contract_and_tokens():
    one, _ = _run([sys.executable, "bench.py", "--gpus", "1", *COMMON, "--full"], {})
    assert one["n_gpus"] == 1 and one["config"]["row_parallel_reduce"] is None
    assert one["config"]["reduced_model"] is True and len(one["config"]["first_step_tokens"]) == 8
    fused, err_f = _torchrun(2, {}, ("--full",))
    plain, _ = _torchrun(2, {"SLM_CUSTOM_AR": "0"}, ("--full",))
    for rec in (fused, plain):
        assert rec["n_gpus"] == 2 and rec["steps"] == 2 and rec["warmup"] == 1
        assert rec["scaling"] == "strong" and rec["unit"] == "tokens/s" and rec["value"] > 0
        assert rec["config"]["parallelism"] == "tp2"
        assert rec["config"]["collectives"]["ranks"] == 2
        assert rec["config"]["collectives"]["backend"] == "gloo"
        assert rec["roofline"]["bound"] == "hbm" and rec["roofline"]["frac"] > 0
        assert rec["cpu_baseline"] is None  # N > 1: no CPU leg
    assert "xgmi" in fused["config"]["row_parallel_reduce"], (fused["config"], err_f[-1500:])
    assert plain["config"]["row_parallel_reduce"] == "gloo all-reduce + rms_norm"
    assert fused["config"]["collectives"]["in_step"].startswith("none")
    t1, tf, tp = (r["config"]["first_step_tokens"] for r in (one, fused, plain))
    assert tf == tp, "fused xGMI reduce and collective + rms_norm must give identical tokens"
    agree = sum(int(a == b) for a, b in zip(t1, tf))
    assert agree >= 6, f"TP=2 reproduces only {agree}/8 of the TP=1 greedy ids: {t1} vs {tf}"


@pytest.mark.timeout(900)
def test_bench_70b_config_reduced_layers_runs_on_one_gpu():
    """BASELINE configs[3] plumbing (Llama-3-70B shapes, GPTQ symmetric g128, bs=128) with the layer
    count cut to 2 so it fits a test: shapes, symmetric zero points, JSON labelling."""
    rec, _ = _run([sys.executable, "bench.py", "--gpus", "1", "--model", "70b", "--layers", "2",
                   "--seqlen", "512", "--steps", "2", "--warmup", "1", "--no-traffic", "--full"], {})
    assert rec["config"]["model"] == "70b" and rec["config"]["global_batch"] == 128
    assert "gptq (symmetric)" in rec["config"]["workload"] and rec["config"]["reduced_model"] is True
    assert rec["int4_gemm"]["shape"] == [128, 8192, 57344]
    assert rec["cpu_baseline"] is None and rec["value"] > 0


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("world,model", [(4, "8b"), (8, "8b"), (8, "70b")])
def test_bench_world_4_and_8_rehearsal_on_one_gpu(world, model):
    """First contact for the driver's N = 4 / 8 runs, as far as one GPU allows (VERDICT r2 item 5 i):
    the same torchrun command with all ranks on this GPU.  Exercises rank indexing at world > 2, one
    KV head per rank at world 8 (both models have 8), the start-up probe (int4 GEMM writing the message
    buffer, then the fused reduce, captured), the buffer alternation of the fused reduce over real
    interprocess mappings at world 4 / 8, and the vocab-sharded greedy exchange.  Fused and collective reduce paths must give
    identical tokens (both sum the `world` partials in fp32 in rank order)."""
    margs = ("--model", model) if model != "8b" else ()
    fused, err_f = _torchrun(world, {}, margs)
    plain, _ = _torchrun(world, {"SLM_CUSTOM_AR": "0"}, margs)
    for rec in (fused, plain):
        assert rec["n_gpus"] == world and rec["config"]["parallelism"] == f"tp{world}"
        assert rec["config"]["collectives"]["ranks"] == world and rec["value"] > 0
        assert rec["config"]["model"] == model
    assert "xgmi" in fused["config"]["row_parallel_reduce"], (fused["config"], err_f[-1500:])
    tf, tp = fused["config"]["first_step_tokens"], plain["config"]["first_step_tokens"]
    assert len(tf) == 8 and tf == tp, f"fused vs collective reduce disagree at world {world}: {tf} vs {tp}"


@pytest.mark.timeout(1800)
def test_bench_two_ranks_with_two_lanes_each_on_one_gpu():
    """Round 5: lanes under TP.  Two ranks on this GPU, each running its shard of a pure-decode batch of 128
    rows as TWO half-batch lanes on two streams, every lane with its OWN instance of the fused all-reduce
    (signal block + alternating message buffers over real interprocess mappings), captured into one
    hipGraph per rank.  The fused reduce raises a sticky error word if a peer never arrives (bench.py
    checks it after the warm-up and after the timed steps), so a protocol mix-up between the lanes'
    instances fails loudly; the tokens must agree with the one-lane TP run up to near-ties (the lanes run
    their GEMMs at half the rows: other split-K / tile plans)."""
    big = ["--layers", "2", "--bs", "128", "--seqlen", "256", "--steps", "2", "--warmup", "1",
           "--no-cpu-baseline", "--no-traffic", "--kv-fill", "consistent"]

    def run(lanes):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "2",
               *big, "--lanes", str(lanes)]
        return _run(cmd, dict(SLM_FORCE_LOCAL_RANK="0", SLM_DIST_BACKEND="gloo"))
    two, err = run(64)
    one, _ = run(0)
    assert "xgmi" in two["config"]["row_parallel_reduce"], (two["config"], err[-1500:])
    assert two["config"]["decode_lanes"] == 2 and one["config"]["decode_lanes"] == 1
    assert two["config"]["hip_graph"] is True
    t2, t1 = two["config"]["first_step_tokens"], one["config"]["first_step_tokens"]
    agree = sum(int(a == b) for a, b in zip(t1, t2))
    assert agree >= 12, f"two lanes per rank reproduce only {agree}/16 of the one-lane TP ids: {t1} vs {t2}"
