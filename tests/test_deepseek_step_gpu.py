"""DeepseekV2DecodeStep (scalellm_amd/deepseek.py) end to end against tests/deepseek_model_ref.py (the torch-fp32
restatement of the DeepSeek-V2 forward with NAIVE attention, pinned on HuggingFace by tests/test_deepseek_ref_cpu.py)
on the step's own checkpoint, dequantised where it is fp8: a prefill step with one sequence chunked, the rest of that
chunk beside decode rows, six decode steps along the reference's greedy path, a captured decode step replayed over
changed lengths, the sampling entry.  bf16, DeepseekV2Shape.tiny(): hidden 256, 4 heads (32 + 64, v 32), latent 128,
3 layers of which the first is dense, 8 routed + 2 shared experts, top 3, vocab 1024; block 16; four prompts of 5 to
40 tokens.

Routing as in tests/test_mixtral_step_gpu.py: the reference runs with the GPU's recorded expert ids forced and
computes its own weights; the router logits, every flip and three controls are checked separately.
Bound: check_logits at 3e-2, the project's bound for a bf16 step against its fp32 reference."""
import numpy as np
import pytest
import torch

from tests import deepseek_model_ref as R
from tests import sampling_ref
from tests.e2e_common import Sequences, check_logits, rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
TOL = 3e-2
BLOCK = 16
PROMPTS = [5, 40, 12, 23]
N_DECODE = 6


def _params(inp):
    from scalellm_amd.layers import InputParameters
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return (t(inp["tokens"]), t(inp["positions"]),
            InputParameters(q_cu_seq_lens=t(inp["q_cu"]), kv_cu_seq_lens=t(inp["kv_cu"]),
                            new_cache_slots=t(inp["slots"]), block_tables=t(inp["table"]),
                            cu_block_lens=t(inp["bcu"]), q_max_seq_len=inp["max_q"], kv_max_seq_len=inp["max_kv"]))


def _dense(sd, name):
    """one checkpoint linear -> the dense fp32 weight [out, in] it stands for"""
    w = sd[name + ".weight"].float().cpu()
    return w * sd[name + ".weight_scale"].float().cpu()[:, None] if name + ".weight_scale" in sd else w


def _reference(model):
    """the restatement over the step's own checkpoint, its embedding and lm_head, and its host-built RoPE table"""
    from scalellm_amd import deepseek
    f = lambda t: t.float().cpu()  # noqa: E731
    s = model.shape
    layers = []
    for li, sd in enumerate(model.ckpt):
        names = ["kv_a_proj_with_mqa", "kv_b_proj", "o_proj"] + (["q_proj"] if s.q_lora_rank is None else
                                                                  ["q_a_proj", "q_b_proj"])
        attn = {n: _dense(sd, "self_attn." + n) for n in names}
        attn["kv_a_layernorm"] = f(sd["self_attn.kv_a_layernorm.weight"])
        if s.q_lora_rank is not None:
            attn["q_a_layernorm"] = f(sd["self_attn.q_a_layernorm.weight"])
        W = {"attn": attn, "in_norm": f(sd["input_layernorm.weight"]),
             "post_norm": f(sd["post_attention_layernorm.weight"])}
        if "mlp.gate.weight" in sd:
            E = s.n_routed_experts
            W["router"] = f(sd["mlp.gate.weight"])
            for ours, hf in (("w1", "gate_proj"), ("w3", "up_proj"), ("w2", "down_proj")):
                W[ours] = torch.stack([_dense(sd, f"mlp.experts.{e}.{hf}") for e in range(E)]).contiguous()
                W["shared_" + hf.split("_")[0]] = _dense(sd, "mlp.shared_experts." + hf)
        else:
            W.update(gate=_dense(sd, "mlp.gate_proj"), up=_dense(sd, "mlp.up_proj"), down=_dense(sd, "mlp.down_proj"))
        layers.append(W)
    table = deepseek.rope_cos_sin_table(s, "cpu")
    half = s.rope_head_dim // 2
    mla = R.MLAConfig(n_heads=s.n_heads, nope=s.nope_head_dim, rope=s.rope_head_dim, v_dim=s.v_head_dim,
                      latent=s.kv_lora_rank, q_lora_rank=s.q_lora_rank, eps=s.rms_eps,
                      sm_scale=deepseek.attention_sm_scale(s), interleaved=True)
    return R.DeepseekV2Ref(layers, f(model.final_norm), f(model.embed), f(model.lm_head),
                           table[:, :half].contiguous(), table[:, half:].contiguous(),
                           R.DeepseekRefConfig(mla=mla, topk=s.topk, rms_eps=s.rms_eps, norm_topk_prob=s.norm_topk_prob))


class _Routing:
    """what the GPU routed, per sequence, sparse layer and position: the forced selection of the reference"""

    def __init__(self, n_seqs, n_layers):
        self.ids = [[[] for _ in range(n_layers)] for _ in range(n_seqs)]

    def record(self, model, new_lens):
        T = sum(new_lens)
        for li, r in enumerate(model.routing):
            ids, w = r["indices"][:T].cpu().numpy(), r["weights"][:T].cpu().numpy()
            assert ids.min() >= 0 and ids.max() < model.shape.n_routed_experts
            assert (w[:, :-1] >= w[:, 1:]).all() and (w > 0).all() and (w.sum(-1) <= 1 + 1e-6).all()
            row = 0
            for s, n in enumerate(new_lens):
                self.ids[s][li] += list(ids[row:row + n])
                row += n

    def forced(self, s, rotate=0, E=8):
        return [(np.stack(rows) + rotate) % E for rows in self.ids[s]]


def _ref_rows(ref, seqs, new_lens, routing, rotate=0):
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


def _run_schedule(shape, quant_method, steps, seed, controls):
    from scalellm_amd.deepseek import DeepseekV2DecodeStep
    seqs = Sequences(PROMPTS, N_DECODE + 4, BLOCK, 1024, seed=13)
    model = DeepseekV2DecodeStep(shape, sum(PROMPTS) + 8, seqs.n_blocks, BLOCK, quant_method=quant_method,
                                 dtype=torch.bfloat16, device=DEV, seed=seed, keep_checkpoint=True, record_routing=True)
    ref = _reference(model)
    ctrl = {}
    if controls:
        ones = [dict(W, attn=dict(W["attn"], kv_a_layernorm=torch.ones_like(W["attn"]["kv_a_layernorm"])))
                for W in ref.layers]
        ctrl = {"no_shared": (ref.variant(shared_experts=False), 0), "rotated": (ref, 1),
                "latent_norm_ones": (ref.variant(layers=ones), 0)}
    routing = _Routing(len(PROMPTS), len(model.sparse_layers))
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
        for name, (variant, rot) in ctrl.items():
            rec[name] = _ref_rows(variant, seqs, new_lens, routing, rotate=rot)[0]
        records.append(rec)
        seqs.advance(new_lens)
        seqs.feed(inp, want.argmax(-1))                            # the REFERENCE's greedy path
    return model, ref, seqs, routing, records


def _tiny():
    from scalellm_amd.deepseek import DeepseekV2Shape
    return DeepseekV2Shape.tiny()


@pytest.fixture(scope="module")
def run():
    """the whole schedule of the unquantised step, run once"""
    first = list(PROMPTS)
    first[1] = 20                                                  # sequence 1 is chunked: 20 now, 20 with step 1
    steps = [first, [1 if i != 1 else PROMPTS[1] - 20 for i in range(len(PROMPTS))]] + [[1] * len(PROMPTS)] * N_DECODE
    return _run_schedule(_tiny(), "none", steps, seed=3, controls=True)


def _check_router(records, what):
    for li in range(len(records[0]["router"])):
        g = np.concatenate([r["gpu_router"][li] for r in records])
        w = np.concatenate([r["router"][li] for r in records])
        rel = rel_l2(g, w)
        print(f"\n[deepseek-step] {what} sparse layer {li}: router logits rel L2 {rel:.4f} over {g.shape[0]} tokens")
        assert np.isfinite(g).all() and rel <= TOL, (what, li, rel)


def test_prefill_chunk_and_decode_logits_match_the_reference(run):
    _, _, _, _, records = run
    for si, r in enumerate(records):
        a, n, rel = check_logits(r["got"], r["want"], TOL, f"step {si} (q_lens {r['new_lens']})")
        print(f"\n[deepseek-step] step {si} q_lens {r['new_lens']} kv {r['kv']}: rel L2 {rel:.4f}, greedy {a}/{n}")
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
    print(f"\n[deepseek-step] {flips} flipped selections in {tokens} (token, sparse layer) routings")
    assert tokens == 2 * sum(sum(r["new_lens"]) for r in records) > 2 * sum(PROMPTS)   # every token, both sparse layers


def test_the_comparison_sees_shared_experts_routing_and_the_latent_norm(run):
    """the same GPU logits against the restatement without the shared experts, with the forced expert ids rotated
    by one, and with kv_a_layernorm's weight replaced by ones, exceed the bound the true reference meets"""
    _, _, _, _, records = run
    got = np.concatenate([r["got"] for r in records])
    for control in ("no_shared", "rotated", "latent_norm_ones"):
        rel = rel_l2(got, np.concatenate([r[control] for r in records]))
        print(f"\n[deepseek-step] control {control}: rel L2 {rel:.4f} (bound {TOL})")
        assert rel > TOL, control
    assert rel_l2(got, np.concatenate([r["want"] for r in records])) <= TOL


@pytest.mark.parametrize("variant", ["qlora", "fp8", "yarn"])
def test_other_configurations_match_the_reference(variant):
    """tiny_qlora(), quant_method="fp8" against the dequantised checkpoint, and the yarn table: one prefill and one
    decode step each"""
    from scalellm_amd.deepseek import DeepseekV2Shape
    shape = DeepseekV2Shape.tiny_qlora() if variant == "qlora" else _tiny()
    if variant == "yarn":
        shape.rope_type, shape.rope_factor, shape.original_max_position = "yarn", 8.0, 64
        shape.mscale, shape.mscale_all_dim = 0.707, 1.0
    steps = [list(PROMPTS), [1] * len(PROMPTS)]
    model, _, _, _, records = _run_schedule(shape, "fp8" if variant == "fp8" else "none", steps, seed=5, controls=False)
    if variant == "fp8":
        from scalellm_amd import layers, moe
        assert isinstance(model.layers[1]["moe"].experts, moe.MoEFp8Experts)
        assert isinstance(model.layers[0]["attn"].qkv_a, layers.ColumnParallelFp8Linear)
        assert model.layers[0]["attn"].kv_b.dtype == torch.bfloat16             # dequantised once at load
    for si, r in enumerate(records):
        a, n, rel = check_logits(r["got"], r["want"], TOL, f"{variant} step {si}")
        print(f"\n[deepseek-step] {variant} step {si} q_lens {r['new_lens']}: rel L2 {rel:.4f}, greedy {a}/{n}")
    _check_router(records, variant)


def test_captured_decode_step_replays_over_changed_lengths(run):
    from scalellm_amd.layers import InputParameters
    model, _, seqs, _, _ = run
    n = len(PROMPTS)
    ones = [1] * n
    inp = seqs.inputs(ones)
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


def test_more_than_one_rank_and_group_limited_routing_are_refused():
    from scalellm_amd.deepseek import DeepseekV2DecodeStep
    from scalellm_amd.model_parallel import ParallelArgs
    with pytest.raises(ValueError):
        DeepseekV2DecodeStep(_tiny(), 8, 4, BLOCK, parallel_args=ParallelArgs(rank=0, world_size=2), device=DEV)
    with pytest.raises(ValueError):
        DeepseekV2DecodeStep(_tiny(), 8, 4, BLOCK, custom_allreduce=object(), device=DEV)
    grouped = _tiny()
    grouped.topk_method = "group_limited_greedy"
    with pytest.raises(ValueError, match="group_limited_greedy"):
        DeepseekV2DecodeStep(grouped, 8, 4, BLOCK, device=DEV)
