"""layers.MLAAttention on a paged latent cache (block 16) against the naive fp32 form of tests/deepseek_model_ref.py:
a prefill with one sequence chunked, the rest of that chunk beside decode rows, then decode steps; bf16; with and
without q_lora_rank.

The bound is not a constant.  On the same inputs the torch bf16 composition of the SAME absorbed arithmetic
(mla_absorbed with a bf16 round trip wherever the kernel path stores a tensor: the projections, the normalised
latent, the rotated values, q_lat, out_lat, v, o) is measured against the fp32 reference, and the kernel path, which
differs from that composition only in the order of its accumulations, is allowed twice that figure.  Both are
printed.  Control: the reference with the value projections of two heads exchanged must exceed the bound."""
import numpy as np
import pytest
import torch

from tests import deepseek_model_ref as R
from tests.e2e_common import Sequences, rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
BLOCK, HIDDEN, MAX_POS = 16, 256, 128
PROMPTS = [5, 40, 12, 23]
N_DECODE = 3


def _params(inp):
    from scalellm_amd.layers import InputParameters
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return t(inp["positions"]), InputParameters(
        q_cu_seq_lens=t(inp["q_cu"]), kv_cu_seq_lens=t(inp["kv_cu"]), new_cache_slots=t(inp["slots"]),
        block_tables=t(inp["table"]), cu_block_lens=t(inp["bcu"]), q_max_seq_len=inp["max_q"],
        kv_max_seq_len=inp["max_kv"])


@pytest.mark.parametrize("q_lora_rank,defer,split", [(None, True, 2), (None, True, None), (None, False, None),
                                                     (64, True, None)])
def test_mla_attention_matches_the_naive_reference(q_lora_rank, defer, split):
    """split: SLM_LINEAR_SPLITK forced, so that the fused [q | c | k_pe] GEMM (K = 256: two chunks of 128) really
    leaves slabs for the prologue's slab form at this small K -- asserted below; the o projection (K = 128, one
    chunk) cannot split here, its deferred path is the caller's and is covered by the step test's shapes"""
    from scalellm_amd import kernels
    from scalellm_amd.layers import HipAttnHandler, LatentKVCache, MLAAttention
    cfg = R.MLAConfig(n_heads=4, nope=32, rope=64, v_dim=32, latent=128, q_lora_rank=q_lora_rank)
    W = R.random_mla_weights(cfg, HIDDEN, seed=21)
    W = {k: R.bf16_round(v) for k, v in W.items()}                 # the checkpoint IS bf16: both sides get these
    total = [n + N_DECODE for n in PROMPTS]
    g = torch.Generator().manual_seed(5)
    xs = [R.bf16_round(torch.randn(n, HIDDEN, generator=g)) for n in total]
    cos, sin = R.default_cos_sin(MAX_POS, cfg.rope)

    seqs = Sequences(PROMPTS, N_DECODE + 1, BLOCK, 16, seed=3)
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, cfg.rope, 2, dtype=torch.float32, device=DEV) / cfg.rope))
    table = HipAttnHandler.build_cos_sin(cfg.rope, MAX_POS, inv_freq)
    attn = MLAAttention(HIDDEN, cfg.n_heads, cfg.nope, cfg.rope, cfg.v_dim, cfg.latent, q_lora_rank, table, True,
                        cfg.scale, cfg.eps, max_tokens=sum(PROMPTS), dtype=torch.bfloat16, device=DEV)
    sd = {k + (".weight" if not k.endswith("weight") else ""): v.to(torch.bfloat16) for k, v in W.items()}
    attn.load_state_dict(sd)
    attn.verify_loaded_weights()
    assert attn.w_uv.data_ptr() == attn.kv_b.data_ptr() + cfg.nope * cfg.latent * 2      # a view, not a copy
    assert attn.w_uv.stride(0) == (cfg.nope + cfg.v_dim) * cfg.latent
    cache = LatentKVCache(seqs.n_blocks, BLOCK, cfg.latent, cfg.rope, torch.bfloat16, DEV)

    first = list(PROMPTS)
    first[1] = 20                                                  # sequence 1 is chunked
    steps = [first, [1 if i != 1 else PROMPTS[1] - 20 for i in range(len(PROMPTS))]] + \
        [[1] * len(PROMPTS)] * (N_DECODE - 1)
    got = [torch.zeros(n, HIDDEN) for n in total]
    done = [0] * len(PROMPTS)
    deferred = []
    for new_lens in steps:
        for s, n in enumerate(new_lens):                           # Sequences wants the tokens to exist
            while len(seqs.tokens[s]) < seqs.cached[s] + n:
                seqs.tokens[s].append(0)
        inp = seqs.inputs(new_lens)
        positions, params = _params(inp)
        x = torch.cat([xs[s][seqs.cached[s]:seqs.cached[s] + n] for s, n in enumerate(new_lens)])
        x = x.to(DEV, torch.bfloat16)
        o = torch.full((x.size(0), HIDDEN), float("nan"), device=DEV, dtype=torch.bfloat16)
        with kernels.tuning(SLM_LINEAR_SPLITK=split):
            attn.forward(x, positions, cache, params, out=o, defer_splitk=defer)
        if attn.o.deferred:                                        # the caller's reduction: here the plain one
            o = _reduce(attn.o.deferred, o)
        deferred.append((bool(attn.qkv_a.deferred) if attn.qkv_a is not None else False, bool(attn.o.deferred)))
        torch.cuda.synchronize()
        row = 0
        for s, n in enumerate(new_lens):
            got[s][seqs.cached[s]:seqs.cached[s] + n] = o[row:row + n].float().cpu()
            row += n
            done[s] = seqs.cached[s] + n
        seqs.advance(new_lens)
    n_done = done
    if split:
        assert any(q for q, _ in deferred), "no step went through the prologue's slab form"
    if not defer:
        assert not any(a or b for a, b in deferred)
    assert all(d > p for d, p in zip(done, PROMPTS))               # every sequence decoded past its prompt

    want, twin, swapped = [], [], []
    for s, n in enumerate(n_done):
        x, c, sn = xs[s][:n], cos[:n], sin[:n]
        want.append(R.mla_naive(x, W, cfg, c, sn))
        twin.append(R.mla_absorbed(x, W, cfg, c, sn, rnd=R.bf16_round))
        swapped.append(R.mla_naive(x, W, cfg, c, sn, swap_uv=(0, 1)))
    cat = lambda xs_: torch.cat(xs_).numpy()  # noqa: E731
    g_all = cat([got[s][:n] for s, n in enumerate(n_done)])
    e_twin = rel_l2(cat(twin), cat(want))
    e_gpu = rel_l2(g_all, cat(want))
    e_ctrl = rel_l2(g_all, cat(swapped))
    print(f"\n[mla-attn] q_lora {q_lora_rank} defer {defer} split {split} (deferred per step {deferred}): torch bf16 composition "
          f"{e_twin:.5f}, kernel path {e_gpu:.5f} (bound {2 * e_twin:.5f}), heads' W_UV swapped {e_ctrl:.5f}")
    assert np.isfinite(g_all).all()
    assert 0 < e_twin < 0.05, "the bf16 composition itself is off: the bound would mean nothing"
    assert e_gpu <= 2 * e_twin
    assert e_ctrl > 2 * e_twin


def _reduce(partials, like):
    """T(sum of the o projection's deferred slabs) through the kernel that consumes them in a step: RMSNorm with a
    unit weight would normalise, so use the residual output of rms_norm(residual=0): residual := T(0 + sum)"""
    from scalellm_amd import kernels
    res = torch.zeros_like(like)
    kernels.rms_norm(torch.empty_like(like), like, torch.ones(like.size(1), device=like.device, dtype=like.dtype),
                     1e-6, residual=res, partials=partials)
    return res


def test_latent_cache_and_layer_refuse_what_they_do_not_support():
    from scalellm_amd.layers import MLAAttention
    from scalellm_amd.model_parallel import ParallelArgs
    table = torch.zeros(8, 64, device=DEV)
    with pytest.raises(ValueError):
        MLAAttention(256, 4, 32, 64, 32, 128, None, table, True, 0.1, 1e-6, 8,
                     parallel_args=ParallelArgs(rank=0, world_size=2), device=DEV)
    with pytest.raises(ValueError):
        MLAAttention(256, 4, 32, 64, 32, 128, None, table, True, 0.1, 1e-6, 8, quant_method="awq", device=DEV)
