"""MixtralDecodeStep / Qwen3DecodeStep(quant_method="fp8", act_quant="fp8"): a prefill step, then the captured decode
step of tests/test_moe_mxfp4_step_gpu.py replayed over changed lengths (finite logits, replay == eager bit for bit)."""
import pytest
import torch

from tests import test_moe_mxfp4_step_gpu as base
from tests.e2e_common import Sequences

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["mixtral-tiny", "qwen3-tiny_moe"])
def test_w8a8_step_is_finite_and_replays_bit_for_bit(name):
    cls, shape = base._family(name)
    for method, act in (("mxfp4", "fp8"), ("none", "fp8"), ("fp8", "int8")):
        with pytest.raises(ValueError, match="act_quant"):
            cls(shape, 8, 4, base.BLOCK, quant_method=method, act_quant=act, dtype=base.DT, device=base.DEV)
    seqs = Sequences(base.PROMPTS, 8, base.BLOCK, 1024, seed=13)
    model = cls(shape, sum(base.PROMPTS) + 8, seqs.n_blocks, base.BLOCK, quant_method="fp8", act_quant="fp8",
                dtype=base.DT, device=base.DEV, seed=4)
    assert all(L["moe"].act_quant == "fp8" and L["qkv"].act_quant == "fp8" for L in model.layers)
    inp = seqs.inputs(list(base.PROMPTS))
    logits = model.forward(*base._params(inp), return_logits=True)
    assert logits.shape == (len(base.PROMPTS), shape.vocab) and bool(torch.isfinite(logits.float()).all())
    assert float(logits.float().abs().max()) > 0                   # finite and not all zero
    seqs.advance(list(base.PROMPTS))
    seqs.feed(inp, logits.float().cpu().numpy().argmax(-1))
    base.test_captured_decode_step_replays_over_changed_lengths((None, model, None, seqs, None))
