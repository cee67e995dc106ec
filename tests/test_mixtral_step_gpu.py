"""MixtralDecodeStep (scalellm_amd/mixtral.py) end to end against tests/mixtral_model_ref.py (the torch-fp32
restatement of the Mixtral forward, pinned on HuggingFace by tests/test_moe_router_cpu.py) on the step's own
checkpoint, dequantised where it is quantised: a prefill step with one sequence chunked, the rest of that chunk beside
decode rows, six decode steps along the reference's greedy path, a captured decode step replayed over changed
lengths, the sampling entry.  bf16, MixtralShape.tiny(): hidden 256, 8 heads x 32, 2 KV heads, intermediate 512,
2 layers, vocab 1024, 8 experts, top 2; block 16; four prompts of 5 to 40 tokens.

Routing.  A bf16 router and an fp32 one disagree on near-ties, and one flipped expert changes a token's FFN output by
its own size.  So the reference runs with the GPU's recorded expert ids forced (record_routing) and computes ITS OWN
weights from ITS OWN router logits at those experts: every token stays in every comparison and nothing is capped.
What the forcing could hide is checked separately: the router logits themselves (relative L2 per layer), every flip
(it must be explained by the two logit errors), and two controls that show the comparison sees the MoE at all.

Bound: check_logits at 3e-2, what tests/test_e2e_gpu.py allows the bf16 Llama step against its fp32 oracle."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import mixtral_model_ref as R
from tests import sampling_ref
from tests.e2e_common import Sequences, check_logits, rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
TOL = 3e-2
BLOCK, GROUP = 16, 128
PROMPTS = [5, 40, 12, 23]
N_DECODE = 6


def _shape():
    from scalellm_amd.mixtral import MixtralShape
    return MixtralShape.tiny()


def _params(inp):
    from scalellm_amd.layers import InputParameters
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return (t(inp["tokens"]), t(inp["positions"]),
            InputParameters(q_cu_seq_lens=t(inp["q_cu"]), kv_cu_seq_lens=t(inp["kv_cu"]),
                            new_cache_slots=t(inp["slots"]), block_tables=t(inp["table"]),
                            cu_block_lens=t(inp["bcu"]), q_max_seq_len=inp["max_q"], kv_max_seq_len=inp["max_kv"]))


def _dense_nk(t, dtype):
    """one checkpoint linear -> the dense fp32 weight [N, K] it stands for"""
    if "qweight" in t:
        return torch.from_numpy(oracle.awq_dequant(t["qweight"].cpu().numpy(), t["qzeros"].cpu().numpy(),
                                                   t["scales"].to(dtype).float().cpu().numpy(), GROUP, bits=4)).t()
    w = t["weight"].float().cpu()
    return w * t["weight_scale"].float().cpu()[:, None] if "weight_scale" in t else w


def _reference(model):
    """the restatement over the step's own checkpoint, its norm weights, embedding and lm_head"""
    f = lambda t: t.float().cpu()  # noqa: E731
    E = model.shape.n_experts
    layers = []
    for li, ck in enumerate(model.ckpt):
        sd = ck["moe"]
        expert = lambda e, w: _dense_nk({k[len(f"experts.{e}.{w}."):]: v for k, v in sd.items()  # noqa: E731
                                         if k.startswith(f"experts.{e}.{w}.")}, model.dtype)
        W = {"qkv": _dense_nk(ck["qkv"], model.dtype).t().contiguous(),
             "o": _dense_nk(ck["o"], model.dtype).t().contiguous(), "gate": f(sd["gate.weight"])}
        for w in ("w1", "w3", "w2"):
            W[w] = torch.stack([expert(e, w) for e in range(E)]).contiguous()
        W["in_norm"], W["post_norm"] = f(model.layers[li]["in_norm"]), f(model.layers[li]["post_norm"])
        layers.append(W)
    s = model.shape
    return R.MixtralRef(layers, f(model.final_norm), f(model.embed), f(model.lm_head), R.MixtralRefConfig(
        n_heads=s.n_heads, n_kv_heads=s.n_kv_heads, head_dim=s.head_dim, topk=s.topk, rms_eps=s.rms_eps,
        rope_theta=s.rope_theta))


class _Routing:
    """what the GPU routed, per sequence, layer and position: the forced selection of the reference"""

    def __init__(self, n_seqs, n_layers):
        self.ids = [[[] for _ in range(n_layers)] for _ in range(n_seqs)]
        self.logits = [[[] for _ in range(n_layers)] for _ in range(n_seqs)]

    def record(self, model, new_lens):
        T = sum(new_lens)
        for li, r in enumerate(model.routing):
            ids, lg = r["indices"][:T].cpu().numpy(), r["logits"][:T].cpu().numpy()
            w = r["weights"][:T].cpu().numpy()
            assert ids.min() >= 0 and ids.max() < model.shape.n_experts
            # renormalised (two fp32 quotients and their sum: a few 2^-24), in descending order
            assert np.allclose(w.sum(-1), 1.0, rtol=0, atol=1e-6) and (w[:, 0] >= w[:, 1]).all()
            row = 0
            for s, n in enumerate(new_lens):
                self.ids[s][li] += list(ids[row:row + n])
                self.logits[s][li] += list(lg[row:row + n])
                row += n

    def forced(self, s, rotate=0, E=8):
        return [(np.stack(rows) + rotate) % E for rows in self.ids[s]]


def _ref_rows(ref, seqs, new_lens, routing, rotate=0):
    """the reference's logits at the last new token of every sequence in the step ([rows, vocab]), and per layer its
    router logits at the step's new tokens ([T, E], rows in the step's order)"""
    rows, router = [], None
    for s, n in enumerate(new_lens):
        if not n:
            continue
        c = seqs.cached[s]
        lg, rt = ref.logits(seqs.tokens[s][:c + n], forced=routing.forced(s, rotate), return_router=True)
        rows.append(lg[-1].numpy())
        new = [r[c:c + n].numpy() for r in rt]
        router = new if router is None else [np.concatenate([a, b]) for a, b in zip(router, new)]
    return np.stack(rows), router


def _run_schedule(quant_method, steps, seed, controls):
    from scalellm_amd.mixtral import MixtralDecodeStep
    seqs = Sequences(PROMPTS, N_DECODE + 4, BLOCK, 1024, seed=13)
    model = MixtralDecodeStep(_shape(), sum(PROMPTS) + 8, seqs.n_blocks, BLOCK, quant_method=quant_method,
                              group_size=GROUP, dtype=torch.bfloat16, device=DEV, seed=seed, keep_checkpoint=True,
                              record_routing=True)
    ref = _reference(model)
    no_renorm = ref.variant(renormalize=False)
    routing = _Routing(len(PROMPTS), model.shape.n_layers)
    records = []
    for new_lens in steps:
        inp = seqs.inputs(new_lens)
        tokens, positions, params = _params(inp)
        logits = model.forward(tokens, positions, params, return_logits=True)
        torch.cuda.synchronize()
        routing.record(model, new_lens)
        T = sum(new_lens)
        want, router = _ref_rows(ref, seqs, new_lens, routing)
        rec = dict(new_lens=new_lens, got=logits.float().cpu().numpy(), want=want, router=router,
                   gpu_router=[r["logits"][:T].cpu().numpy() for r in model.routing],
                   gpu_ids=[r["indices"][:T].cpu().numpy() for r in model.routing],
                   kv=[seqs.cached[s] + n for s, n in enumerate(new_lens)])
        if controls:
            rec["no_renorm"] = _ref_rows(no_renorm, seqs, new_lens, routing)[0]
            rec["rotated"] = _ref_rows(ref, seqs, new_lens, routing, rotate=1)[0]
        records.append(rec)
        seqs.advance(new_lens)
        seqs.feed(inp, want.argmax(-1))                            # the REFERENCE's greedy path
    return model, ref, seqs, routing, records


@pytest.fixture(scope="module")
def run():
    """the whole schedule of the unquantised step, run once"""
    first = list(PROMPTS)
    first[1] = 20                                                  # sequence 1 is chunked: 20 now, 20 with step 1
    steps = [first, [1 if i != 1 else PROMPTS[1] - 20 for i in range(len(PROMPTS))]] + [[1] * len(PROMPTS)] * N_DECODE
    return _run_schedule("none", steps, seed=3, controls=True)


def _check_router(records, what):
    n_layers = len(records[0]["router"])
    for li in range(n_layers):
        g = np.concatenate([r["gpu_router"][li] for r in records])
        w = np.concatenate([r["router"][li] for r in records])
        rel = rel_l2(g, w)
        print(f"\n[mixtral-step] {what} layer {li}: router logits rel L2 {rel:.4f} over {g.shape[0]} tokens")
        assert np.isfinite(g).all() and rel <= TOL, (what, li, rel)


def test_prefill_chunk_and_decode_logits_match_the_reference(run):
    _, _, _, _, records = run
    agree = total = 0
    for si, r in enumerate(records):
        a, n, rel = check_logits(r["got"], r["want"], TOL, f"step {si} (q_lens {r['new_lens']})")
        print(f"\n[mixtral-step] step {si} q_lens {r['new_lens']} kv {r['kv']}: rel L2 {rel:.4f}, greedy {a}/{n}")
        agree, total = agree + a, total + n
    assert len(records) == 2 + N_DECODE and max(r["new_lens"][1] for r in records[:2]) == 20


def test_router_logits_match_the_reference(run):
    _check_router(run[4], "none")


def test_every_flip_is_explained_by_the_two_logit_errors(run):
    """wherever the reference's free top-k differs from the GPU's: a GPU-chosen expert a displaced b, so
    g[a] >= g[b] while r[b] >= r[a], hence r[b] - r[a] <= |g[a] - r[a]| + |g[b] - r[b]|"""
    _, _, _, _, records = run
    flips = tokens = 0
    for r in records:
        for li, (ref_r, g, ids) in enumerate(zip(r["router"], r["gpu_router"], r["gpu_ids"])):
            free = R.free_topk(torch.from_numpy(ref_r), ids.shape[1]).numpy()
            for t in range(ids.shape[0]):
                tokens += 1
                gpu_set, ref_set = set(ids[t].tolist()), set(free[t].tolist())
                if gpu_set == ref_set:
                    continue
                flips += 1
                for a in gpu_set - ref_set:
                    for b in ref_set - gpu_set:
                        gap = float(ref_r[t, b]) - float(ref_r[t, a])
                        errs = abs(float(g[t, a]) - float(ref_r[t, a])) + abs(float(g[t, b]) - float(ref_r[t, b]))
                        assert gap <= errs, (li, t, a, b, gap, errs)
    print(f"\n[mixtral-step] {flips} flipped selections in {tokens} (token, layer) routings")
    assert tokens == 2 * sum(sum(r["new_lens"]) for r in records) > 2 * sum(PROMPTS)   # every token, both layers


def test_the_comparison_sees_the_mixture_of_experts(run):
    """the same GPU logits against the restatement without the renormalisation, and with the forced expert ids
    rotated by one, exceed the bound the true reference meets"""
    _, _, _, _, records = run
    got = np.concatenate([r["got"] for r in records])
    for control in ("no_renorm", "rotated"):
        rel = rel_l2(got, np.concatenate([r[control] for r in records]))
        print(f"\n[mixtral-step] control {control}: rel L2 {rel:.4f} (bound {TOL})")
        assert rel > TOL, control
    assert rel_l2(got, np.concatenate([r["want"] for r in records])) <= TOL


@pytest.mark.parametrize("quant_method", ["fp8", "awq"])
def test_quantised_steps_match_the_reference_on_the_dequantised_checkpoint(quant_method):
    steps = [list(PROMPTS), [1] * len(PROMPTS)]                    # one prefill, one decode step
    model, _, _, _, records = _run_schedule(quant_method, steps, seed=5, controls=False)
    from scalellm_amd import moe
    assert isinstance(model.layers[0]["moe"].experts,
                      moe.MoEFp8Experts if quant_method == "fp8" else moe.MoEQuantExperts)
    for si, r in enumerate(records):
        a, n, rel = check_logits(r["got"], r["want"], TOL, f"{quant_method} step {si}")
        print(f"\n[mixtral-step] {quant_method} step {si} q_lens {r['new_lens']}: rel L2 {rel:.4f}, greedy {a}/{n}")
    _check_router(records, quant_method)


def test_captured_decode_step_replays_over_changed_lengths(run):
    from scalellm_amd.layers import InputParameters
    model, _, seqs, _, _ = run
    n = len(PROMPTS)
    ones = [1] * n
    inp = seqs.inputs(ones)
    # static inputs, the block table at its full length (every sequence's blocks for the steps to come)
    full_table = np.concatenate([seqs.blocks[s] * BLOCK for s in range(n)]).astype(np.int32)
    bcu = np.concatenate([[0], np.cumsum([len(seqs.blocks[s]) for s in range(n)])]).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    st = dict(tokens=t(inp["tokens"]), positions=t(inp["positions"]), q_cu=t(inp["q_cu"]), kv_cu=t(inp["kv_cu"]),
              slots=t(inp["slots"]))
    params = InputParameters(q_cu_seq_lens=st["q_cu"], kv_cu_seq_lens=st["kv_cu"], new_cache_slots=st["slots"],
                             block_tables=t(full_table), cu_block_lens=t(bcu), q_max_seq_len=1,
                             kv_max_seq_len=max(len(b) for b in seqs.blocks) * BLOCK, kv_total_len=-1)
    model.reserve_workspaces(n, params.kv_max_seq_len)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm-up (writes this step's KV: harmless, the
        model.forward(st["tokens"], st["positions"], params, return_logits=True)   # replay writes the same rows)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        logits = model.forward(st["tokens"], st["positions"], params, return_logits=True)
    seen = []
    for rep in range(2):                                           # two steps: the lengths change under the graph
        inp = seqs.inputs(ones)
        for k in ("tokens", "positions", "q_cu", "kv_cu", "slots"):
            st[k].copy_(t(inp[k]))
        graph.replay()
        torch.cuda.synchronize()
        got = logits.float().cpu().numpy()
        ids = model.routing[0]["indices"][:n].clone()
        eager = model.forward(st["tokens"], st["positions"], params, return_logits=True).float().cpu().numpy()
        assert np.isfinite(got).all()
        assert np.array_equal(got, eager), "the replay differs from the eager step on the same inputs"
        assert torch.equal(model.routing[0]["indices"][:n], ids)
        seen.append(got)
        seqs.advance(ones)
        seqs.feed(inp, got.argmax(-1))
    assert not np.array_equal(seen[0], seen[1])


def test_sampling_returns_the_reference_sampler_tokens_on_the_logits(run):
    from scalellm_amd.sampling import SamplingParameter, SamplingParameters
    model, _, seqs, _, _ = run
    n = len(PROMPTS)
    inp = seqs.inputs([1] * n)
    tokens, positions, params = _params(inp)
    logits = model.forward(tokens, positions, params, return_logits=True).float().cpu().numpy()
    greedy = model.forward(tokens, positions, params).cpu().numpy()
    assert np.array_equal(greedy, logits.argmax(-1))
    reqs = [SamplingParameter(temperature=0.8, do_sample=r != 2, seed=900 + r) for r in range(n)]
    sp = SamplingParameters.create(reqs, device=DEV, compact=False)
    out = model.forward(tokens, positions, params, sampling=sp)
    torch.cuda.synchronize()
    tok = out.next_tokens.cpu().numpy()
    last_pos = inp["positions"][inp["q_cu"][1:] - 1]
    for r in range(n):
        processed, _ = sampling_ref.process_row(logits[r], temp=0.8)
        if not reqs[r].do_sample:
            assert tok[r] == int(np.argmax(processed)), r
            continue
        s = sampling_ref.race_scores(processed, reqs[r].seed, int(last_pos[r]))
        o = np.argsort(-s.astype(np.float64), kind="stable")
        assert tok[r] == o[0] or (tok[r] == o[1] and s[o[1]] >= s[o[0]] * (1 - 1e-5)), (r, tok[r], o[:2])
    with pytest.raises(ValueError):
        model.forward(tokens, positions, params, return_logits=True, sampling=sp)


def test_more_than_one_rank_is_refused():
    from scalellm_amd.mixtral import MixtralDecodeStep
    from scalellm_amd.model_parallel import ParallelArgs
    with pytest.raises(ValueError):
        MixtralDecodeStep(_shape(), 8, 4, BLOCK, parallel_args=ParallelArgs(rank=0, world_size=2), device=DEV)
    with pytest.raises(ValueError):
        MixtralDecodeStep(_shape(), 8, 4, BLOCK, custom_allreduce=object(), device=DEV)
