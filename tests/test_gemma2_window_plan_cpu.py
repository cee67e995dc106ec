"""The max_kv_len hint of a windowed decode call (kernels.visible_kv_hint) and what the library's launch plan makes of
it, host side only: with the context length as the hint, Gemma-2-9B's attention at batch 1 over a 32 k context is cut
into four times the KV shares the same 4 k window gets at a 4 k context; with the visible length both get one plan."""
import ctypes as C

import pytest

from scalellm_amd import _lib, kernels


def _splits(batch, max_kv_len, window_behind):
    a = _lib.AttnArgs()
    a.dtype = _lib.SLM_BF16
    a.batch_size = a.n_tokens = batch
    a.n_heads, a.n_kv_heads, a.head_dim = 16, 8, 256
    a.block_size, a.max_q_len, a.max_kv_len = 16, 1, max_kv_len
    a.k_stride[0] = a.v_stride[0] = 8 * 256
    a.sm_scale, a.logits_soft_cap, a.sliding_window = 256 ** -0.5, 50.0, window_behind
    return int(_lib.lib().slm_paged_kv_varlen_mha_auto_splits(C.byref(a)))


def test_hint_is_the_visible_length_of_a_pure_decode_call():
    assert kernels.visible_kv_hint(32768, 1, 4095) == 4096
    assert kernels.visible_kv_hint(100, 1, 4095) == 100        # shorter than the window
    assert kernels.visible_kv_hint(32768, 1, -1) == 32768      # no window
    assert kernels.visible_kv_hint(32768, 5, 4095) == 32768    # rows of a prefill chunk: left to the plan
    assert kernels.visible_kv_hint(32768, 1, 0) == 1           # the query's own key alone


@pytest.mark.parametrize("batch", [1, 8, 32])
def test_a_long_context_gets_the_plan_of_its_window(batch):
    behind = 4095
    at_4k = _splits(batch, kernels.visible_kv_hint(4096, 1, behind), behind)
    at_32k = _splits(batch, kernels.visible_kv_hint(32768, 1, behind), behind)
    assert at_32k == at_4k
    assert _splits(batch, 4096, -1) == at_4k                   # and of the same keys without a window
    if batch == 1:
        assert _splits(1, 32768, behind) > at_4k               # what the context length as the hint costs
