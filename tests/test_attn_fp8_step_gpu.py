"""LlamaDecodeStep(kv_cache_dtype="fp8") on the tiny shape (with head_dim 64: the tiny shape's 32 is outside the fp8
attention's 64 / 128 / 256): a prefill and two decode steps against the restatement of
tests/test_dense_step_gpu.py with ONE line added -- K and V are replaced by their dequantised e4m3 codes at the
append -- under that test's tolerances; the cache bytes against quantize_fp8_kv of the restatement's K and V; eager
against graph replay, bit for bit.  The bytes are compared wherever the GPU's rotated bf16 K / V equal the twin's;
the test prints that share of the elements and requires more than 99 %."""
import dataclasses

import pytest
import torch

from tests import e2e_common
from tests.e2e_common import Sequences, check_logits
from tests.test_dense_step_gpu import DEV, _oracle_twin, _params

pytestmark = pytest.mark.gpu


def _kv_scales(n_layers, n_kv_heads):
    return [(torch.tensor([0.02 * (1 + h + li) for h in range(n_kv_heads)]),
             torch.tensor([0.05 / (1 + h + 2 * li) for h in range(n_kv_heads)])) for li in range(n_layers)]


def _requantising(monkeypatch, twins, scales):
    """The one added line: what a twin appends is dequantize(quantize(k)), dequantize(quantize(v)) under its layer's
    scales.  Returns the (layer, k, v) every append of the bf16-storage twin was given."""
    from scalellm_amd import kernels
    plain, seen = e2e_common.oracle.set_kv_cache, []

    def append(slots, k, v, kc, vc):
        tw, li = next((tw, li) for tw in twins for li in range(len(tw.kc)) if tw.kc[li] is kc)
        if tw.storage:
            seen.append((li, k.copy(), v.copy()))
        deq = [kernels.dequantize_fp8_kv(kernels.quantize_fp8_kv(torch.from_numpy(x), s), s).numpy()
               for x, s in zip((k, v), scales[li])]
        plain(slots, deq[0], deq[1], kc, vc)
    monkeypatch.setattr(e2e_common.oracle, "set_kv_cache", append)
    return seen


def test_fp8_kv_step_matches_the_restatement_and_its_graph(monkeypatch):
    from scalellm_amd import kernels
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape, hf_state_dict
    B, prompt_lens = 16, [9, 5, 12]
    shape = dataclasses.replace(LlamaShape.tiny(), head_dim=64)
    scales = _kv_scales(shape.n_layers, shape.n_kv_heads)
    seqs = Sequences(prompt_lens, 4, B, 1024, seed=7)
    model = LlamaDecodeStep(shape, sum(prompt_lens) + 8, seqs.n_blocks, B, quant_method="none", dtype=torch.bfloat16,
                            device=DEV, seed=3, keep_checkpoint=True, kv_cache_dtype="fp8", kv_scales=scales)
    assert model.kv_fp8 and model.lanes_min == 0 and model.layers[0]["kv"].key_cache.dtype == torch.uint8
    sd = hf_state_dict(model)
    assert torch.equal(sd["model.layers.1.self_attn.v_scale"].cpu(), scales[1][1])
    model.load_kv_scales({"model.layers.0.self_attn.k_scale": scales[0][0]})           # the names of the fp8 exports
    ref_model, twin_model = _oracle_twin(model), _oracle_twin(model, storage="bf16")
    seen = _requantising(monkeypatch, (ref_model, twin_model), scales)
    gpu_kv, plain_append = [], kernels.set_kv_cache_fp8
    monkeypatch.setattr(kernels, "set_kv_cache_fp8",
                        lambda s, k, v, *a: (gpu_kv.append((k.clone(), v.clone())), plain_append(s, k, v, *a))[1])
    for L in model.layers:                                                             # NaN codes wherever nothing is appended
        L["kv"].key_cache.fill_(0x7F)
        L["kv"].value_cache.fill_(0x7F)
    same = total = 0
    for step, new_lens in enumerate([prompt_lens, [1, 1, 1], [1, 1, 1]]):
        inp = seqs.inputs(new_lens)
        tokens, positions, params = _params(inp)
        snap = [(L["kv"].key_cache.clone(), L["kv"].value_cache.clone()) for L in model.layers]
        del seen[:], gpu_kv[:]
        logits = model.forward(tokens, positions, params, return_logits=True).clone()
        torch.cuda.synchronize()
        got = logits.float().cpu().numpy()
        check_logits(got, ref_model.forward(inp), 3e-2, f"fp8 KV, step {step}: vs the fp32 restatement")
        check_logits(got, twin_model.forward(inp), 1.5e-2, f"fp8 KV, step {step}: vs the bf16-storage twin")
        # cache bytes = quantize_fp8_kv(the twin's K and V) wherever the GPU's bf16 values equal the twin's
        slots = torch.from_numpy(inp["slots"]).long()
        for (li, k, v), (gk, gv) in zip(seen, gpu_kv):
            kv = model.layers[li]["kv"]
            for x, gx, cache, s in ((k, gk, kv.key_cache, scales[li][0]), (v, gv, kv.value_cache, scales[li][1])):
                x = torch.from_numpy(x)
                agree = gx.float().cpu() == x
                want = kernels.quantize_fp8_kv(x, s).view(torch.uint8)
                assert torch.equal(cache.cpu()[slots][agree], want[agree])
                same, total = same + int(agree.sum()), total + agree.numel()
        if step:   # a decode step: its graph, captured over the restored cache, replays to the eager bits
            for L, (k0, v0) in zip(model.layers, snap):
                L["kv"].key_cache.copy_(k0)
                L["kv"].value_cache.copy_(v0)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = model.forward(tokens, positions, params, return_logits=True)
            for _ in range(2):
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, logits)
        seqs.advance(new_lens)
        seqs.feed(inp, got.argmax(-1))
    print(f"[fp8 KV step] cache bytes compared on {same}/{total} elements ({same / total:.4f})")
    assert same / total > 0.99
