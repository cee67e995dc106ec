"""Gemma2DecodeStep (scalellm_amd/gemma2.py) end to end against tests/gemma2_model_ref.py (the torch-fp32 restatement
of the reference's gemma2.h forward, pinned on HuggingFace by tests/test_gemma2_ref_cpu.py) on the dequantised
checkpoint: prefill, one chunked-prefill step beside decode rows, six decode steps along the reference's greedy
path, and a captured decode step replayed over changed lengths.  bf16.

Tiny configuration: hidden 512, 2 heads x 256, 1 KV head, intermediate 1024, 4 layers, vocab 1024, AWQ g128, window
16, attn_scalar 144 (not head_dim), caps 50 / 30, block 16.  Four prompts of 5 to 40 tokens, so kv crosses W + 1.
Bound: check_logits at 3e-2, what tests/test_e2e_gpu.py allows the bf16 Llama step against its fp32 oracle; every
|logit| <= 30.  Two controls make the comparison discriminate: against the restatement with the window off, and
with sm_scale = head_dim ** -0.5, the same logits must EXCEED the bound."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import gemma2_model_ref as R
from tests import sampling_ref
from tests.e2e_common import Sequences, check_logits, rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
TOL = 3e-2
BLOCK, WINDOW, GROUP = 16, 16, 128
PROMPTS = [5, 40, 12, 23]
N_DECODE = 6


def _shape():
    from scalellm_amd.gemma2 import Gemma2Shape
    return Gemma2Shape(hidden=512, n_heads=2, n_kv_heads=1, head_dim=256, intermediate=1024, n_layers=4, vocab=1024,
                       max_position=512, attn_scalar=144.0, sliding_window=WINDOW, attn_logit_soft_cap=50.0,
                       final_logit_soft_cap=30.0)


def _params(inp):
    from scalellm_amd.layers import InputParameters
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return (t(inp["tokens"]), t(inp["positions"]),
            InputParameters(q_cu_seq_lens=t(inp["q_cu"]), kv_cu_seq_lens=t(inp["kv_cu"]),
                            new_cache_slots=t(inp["slots"]), block_tables=t(inp["table"]),
                            cu_block_lens=t(inp["bcu"]), q_max_seq_len=inp["max_q"], kv_max_seq_len=inp["max_kv"]))


def _reference(model):
    """the restatement over the step's own checkpoint, dequantised as the reference's construct_weights does
    (oracle.awq_dequant), its norm weights and tied embedding, and the T-rounded embedding scale the reference uses"""
    f = lambda t: t.float().cpu()  # noqa: E731
    layers = []
    for li, ck in enumerate(model.ckpt):
        W = {name: torch.from_numpy(oracle.awq_dequant(t["qweight"].cpu().numpy(), t["qzeros"].cpu().numpy(),
                                                       f(t["scales"].to(model.dtype)).numpy(), GROUP, bits=4))
             for name, t in ck.items()}
        for name in ("in_norm", "post_attn_norm", "pre_ffn_norm", "post_ffn_norm"):
            W[name] = f(model.layers[li][name])
        layers.append(W)
    s = model.shape
    return R.Gemma2Ref(layers, f(model.final_norm), f(model.embed), R.Gemma2RefConfig(
        n_heads=s.n_heads, n_kv_heads=s.n_kv_heads, head_dim=s.head_dim, rms_eps=s.rms_eps, rope_theta=s.rope_theta,
        attn_scalar=s.attn_scalar, sliding_window=s.sliding_window, attn_logit_soft_cap=s.attn_logit_soft_cap,
        final_logit_soft_cap=s.final_logit_soft_cap, embed_scale=model.embed_scale))


def _ref_rows(ref, seqs, new_lens):
    """[rows, vocab]: the reference's logits at the last new token of every sequence that takes part in the step"""
    rows = [ref.logits(seqs.tokens[s][:seqs.cached[s] + n])[-1].numpy() for s, n in enumerate(new_lens) if n]
    return np.stack(rows)


@pytest.fixture(scope="module")
def run():
    """the whole schedule, run once: per step (new_lens, GPU logits, reference logits, the two controls' logits)"""
    from scalellm_amd.gemma2 import Gemma2DecodeStep
    seqs = Sequences(PROMPTS, N_DECODE + 4, BLOCK, 1024, seed=13)   # chunk step, decode, 2 replays, sampling
    model = Gemma2DecodeStep(_shape(), sum(PROMPTS) + 8, seqs.n_blocks, BLOCK, quant_method="awq", group_size=GROUP,
                             dtype=torch.bfloat16, device=DEV, seed=3, keep_checkpoint=True)
    ref = _reference(model)
    no_window = ref.variant(sliding_window=-1)
    head_scale = ref.variant(sm_scale=256.0 ** -0.5)
    first = list(PROMPTS)
    first[1] = 20                                                  # sequence 1 is chunked: 20 now, 20 with step 1
    steps = [first, [1 if i != 1 else PROMPTS[1] - 20 for i in range(len(PROMPTS))]] + [[1] * len(PROMPTS)] * N_DECODE
    records = []
    for new_lens in steps:
        inp = seqs.inputs(new_lens)
        tokens, positions, params = _params(inp)
        logits = model.forward(tokens, positions, params, return_logits=True)
        torch.cuda.synchronize()
        want = _ref_rows(ref, seqs, new_lens)
        records.append(dict(new_lens=new_lens, got=logits.float().cpu().numpy(), want=want,
                            no_window=_ref_rows(no_window, seqs, new_lens),
                            head_scale=_ref_rows(head_scale, seqs, new_lens),
                            kv=[seqs.cached[s] + n for s, n in enumerate(new_lens)]))
        seqs.advance(new_lens)
        seqs.feed(inp, want.argmax(-1))                            # the REFERENCE's greedy path
    return model, ref, seqs, records


def test_prefill_chunk_and_decode_logits_match_the_reference(run):
    _, _, _, records = run
    agree = total = 0
    for si, r in enumerate(records):
        a, n, rel = check_logits(r["got"], r["want"], TOL, f"step {si} (q_lens {r['new_lens']})")
        print(f"\n[gemma2-step] step {si} q_lens {r['new_lens']} kv {r['kv']}: rel L2 {rel:.4f}, greedy {a}/{n}")
        agree, total = agree + a, total + n
        assert np.abs(r["got"]).max() <= 30.0
    assert max(max(r["kv"]) for r in records) > WINDOW + 1 and agree >= total - 2


def test_the_comparison_sees_the_window_and_the_attention_scale(run):
    """over the steps whose sequences are longer than W + 1 keys, the same GPU logits against the restatement with
    the window off, and with sm_scale from head_dim, exceed the bound the true reference meets"""
    _, _, _, records = run
    long_steps = [r for r in records if max(r["kv"]) > WINDOW + 1]
    assert long_steps
    got = np.concatenate([r["got"] for r in long_steps])
    for control in ("no_window", "head_scale"):
        rel = rel_l2(got, np.concatenate([r[control] for r in long_steps]))
        print(f"\n[gemma2-step] control {control}: rel L2 {rel:.4f} (bound {TOL})")
        assert rel > TOL, control
    assert rel_l2(got, np.concatenate([r["want"] for r in long_steps])) <= TOL


def test_captured_decode_step_replays_over_changed_lengths(run):
    from scalellm_amd.layers import InputParameters
    model, ref, seqs, _ = run
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
    for rep in range(2):                                           # two steps: the lengths change under the graph
        inp = seqs.inputs(ones)
        for k in ("tokens", "positions", "q_cu", "kv_cu", "slots"):
            st[k].copy_(t(inp[k]))
        graph.replay()
        torch.cuda.synchronize()
        got = logits.float().cpu().numpy()
        want = _ref_rows(ref, seqs, ones)
        _, _, rel = check_logits(got, want, TOL, f"replay {rep}")
        eager = model.forward(st["tokens"], st["positions"], params, return_logits=True).float().cpu().numpy()
        assert np.array_equal(got, eager), "the replay differs from the eager step on the same inputs"
        print(f"\n[gemma2-step] replay {rep} kv {[c + 1 for c in seqs.cached]}: rel L2 {rel:.4f}")
        seqs.advance(ones)
        seqs.feed(inp, want.argmax(-1))


def test_sampling_returns_the_reference_sampler_tokens_on_the_capped_logits(run):
    from scalellm_amd.sampling import SamplingParameter, SamplingParameters
    model, _, seqs, _ = run
    n = len(PROMPTS)
    inp = seqs.inputs([1] * n)
    tokens, positions, params = _params(inp)
    capped = model.forward(tokens, positions, params, return_logits=True).float().cpu().numpy()
    greedy = model.forward(tokens, positions, params).cpu().numpy()
    assert np.abs(capped).max() <= 30.0 and np.array_equal(greedy, capped.argmax(-1))
    reqs = [SamplingParameter(temperature=0.8, do_sample=r != 2, seed=900 + r) for r in range(n)]
    sp = SamplingParameters.create(reqs, device=DEV, compact=False)
    out = model.forward(tokens, positions, params, sampling=sp)
    torch.cuda.synchronize()
    tok = out.next_tokens.cpu().numpy()
    last_pos = inp["positions"][inp["q_cu"][1:] - 1]
    for r in range(n):
        processed, _ = sampling_ref.process_row(capped[r], temp=0.8)
        if not reqs[r].do_sample:
            assert tok[r] == int(np.argmax(processed)), r
            continue
        s = sampling_ref.race_scores(processed, reqs[r].seed, int(last_pos[r]))
        o = np.argsort(-s.astype(np.float64), kind="stable")
        assert tok[r] == o[0] or (tok[r] == o[1] and s[o[1]] >= s[o[0]] * (1 - 1e-5)), (r, tok[r], o[:2])
    with pytest.raises(ValueError):
        model.forward(tokens, positions, params, return_logits=True, sampling=sp)


def test_more_than_one_rank_is_refused():
    from scalellm_amd.gemma2 import Gemma2DecodeStep
    from scalellm_amd.model_parallel import ParallelArgs
    with pytest.raises(ValueError):
        Gemma2DecodeStep(_shape(), 8, 4, BLOCK, parallel_args=ParallelArgs(rank=0, world_size=2), device=DEV)
    with pytest.raises(ValueError):
        Gemma2DecodeStep(_shape(), 8, 4, BLOCK, custom_allreduce=object(), device=DEV)


def test_presets_carry_the_public_configurations():
    from scalellm_amd.gemma2 import Gemma2Shape
    for s, (hidden, heads, kv, d, inter, layers, scalar) in (
            (Gemma2Shape.gemma2_2b(), (2304, 8, 4, 256, 9216, 26, 256)),
            (Gemma2Shape.gemma2_9b(), (3584, 16, 8, 256, 14336, 42, 256)),
            (Gemma2Shape.gemma2_27b(), (4608, 32, 16, 128, 36864, 46, 144))):
        assert (s.hidden, s.n_heads, s.n_kv_heads, s.head_dim, s.intermediate, s.n_layers, s.attn_scalar) == \
            (hidden, heads, kv, d, inter, layers, scalar)
        assert (s.vocab, s.sliding_window, s.attn_logit_soft_cap, s.final_logit_soft_cap, s.rms_eps) == \
            (256000, 4096, 50.0, 30.0, 1e-6)
