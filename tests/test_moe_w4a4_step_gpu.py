"""MixtralDecodeStep / Qwen3DecodeStep(quant_method="mxfp4", act_quant="mxfp4"): a prefill step, then a captured decode
step replayed over changed lengths -- finite logits, replay == eager bit for bit, recorded routing included."""
import numpy as np
import pytest
import torch

from tests.e2e_common import Sequences
from tests.test_moe_mxfp4_step_gpu import BLOCK, DEV, DT, PROMPTS, _family, _params

pytestmark = pytest.mark.gpu


def _routing(model, n):
    return [{k: r[k][:n].clone() for k in ("logits", "indices", "weights")} for r in model.routing]


@pytest.mark.parametrize("name", ["mixtral-tiny", "qwen3-tiny_moe"])
def test_w4a4_step_is_finite_and_replays_bit_for_bit(name):
    from scalellm_amd.layers import InputParameters
    cls, shape = _family(name)
    with pytest.raises(ValueError, match="act_quant"):
        cls(shape, 8, 4, BLOCK, quant_method="fp8", act_quant="mxfp4", dtype=DT, device=DEV)
    seqs = Sequences(PROMPTS, 8, BLOCK, 1024, seed=13)
    model = cls(shape, sum(PROMPTS) + 8, seqs.n_blocks, BLOCK, quant_method="mxfp4", act_quant="mxfp4", dtype=DT,
                device=DEV, seed=4, record_routing=True)
    assert all(L["moe"].act_quant == "mxfp4" and L["qkv"].act_quant == "mxfp4" for L in model.layers)
    n = len(PROMPTS)
    inp = seqs.inputs(list(PROMPTS))
    tokens, positions, params = _params(inp)
    logits = model.forward(tokens, positions, params, return_logits=True)
    assert logits.shape == (n, shape.vocab) and bool(torch.isfinite(logits.float()).all())
    assert float(logits.float().abs().max()) > 0
    seqs.advance(list(PROMPTS))
    seqs.feed(inp, logits.float().cpu().numpy().argmax(-1))

    ones = [1] * n
    inp = seqs.inputs(ones)
    full_table = np.concatenate([seqs.blocks[s] * BLOCK for s in range(n)]).astype(np.int32)
    bcu = np.concatenate([[0], np.cumsum([len(seqs.blocks[s]) for s in range(n)])]).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    st = {k: t(inp[k]) for k in ("tokens", "positions", "q_cu", "kv_cu", "slots")}
    params = InputParameters(q_cu_seq_lens=st["q_cu"], kv_cu_seq_lens=st["kv_cu"], new_cache_slots=st["slots"],
                             block_tables=t(full_table), cu_block_lens=t(bcu), q_max_seq_len=1,
                             kv_max_seq_len=max(len(b) for b in seqs.blocks) * BLOCK, kv_total_len=-1)
    model.reserve_workspaces(n, params.kv_max_seq_len)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.forward(st["tokens"], st["positions"], params, return_logits=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.forward(st["tokens"], st["positions"], params, return_logits=True)
    seen = []
    for _ in range(2):                                             # the lengths change under the graph
        inp = seqs.inputs(ones)
        for k in st:
            st[k].copy_(t(inp[k]))
        graph.replay()
        torch.cuda.synchronize()
        got, got_routing = out.clone(), _routing(model, n)
        eager = model.forward(st["tokens"], st["positions"], params, return_logits=True)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got.float()).all()) and torch.equal(got, eager)
        for rg, re_ in zip(got_routing, _routing(model, n)):
            assert all(torch.equal(rg[k], re_[k]) for k in rg)
        seen.append(got)
        seqs.advance(ones)
        seqs.feed(inp, got.float().cpu().numpy().argmax(-1))
    assert not torch.equal(seen[0], seen[1])
