"""CPU tests of the fp8 KV cache boundary (include/slm_hip.h section 27): the argument block against the header, every
refusal before a launch, the plan's workspace against the documented partial layout, and the torch helpers."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

from scalellm_amd import _lib, kernels
from scalellm_amd._lib import AttnFp8Args, AttnFp8PlanInfo

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slm_hip.h")
INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT, SHAPE = -1, -2, -3, -5, -6
P = 1 << 20   # a 16-byte aligned stand-in for every pointer: nothing below launches


def _args(n_tokens=4, n_heads=8, n_kv_heads=2, head_dim=128, **over):
    a = AttnFp8Args()
    for f in ("out", "query", "key_cache", "value_cache", "q_cu_lens", "kv_cu_lens", "block_table", "block_cu_lens",
              "k_scale", "v_scale"):
        setattr(a, f, P)
    a.o_stride[0] = a.q_stride[0] = n_heads * head_dim
    a.o_stride[1] = a.q_stride[1] = a.k_stride[1] = a.v_stride[1] = head_dim
    a.k_stride[0] = a.v_stride[0] = n_kv_heads * head_dim
    a.dtype, a.batch_size, a.n_tokens = _lib.SLM_BF16, n_tokens, n_tokens
    a.n_heads, a.n_kv_heads, a.head_dim, a.block_size = n_heads, n_kv_heads, head_dim, 16
    a.max_q_len, a.max_kv_len, a.sm_scale, a.sliding_window = 1, 4096, 0.1, -1
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def _plan(a):
    info = AttnFp8PlanInfo()
    return _lib.lib().slm_paged_kv_fp8_attention_plan(C.byref(a), C.byref(info)), info


def test_the_argument_blocks_match_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    structs = {"slm_attn_fp8_args": AttnFp8Args, "slm_attn_fp8_plan_info": AttnFp8PlanInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {']
    for cname, ct in structs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in ct._fields_]
    (tmp_path / "abi.c").write_text("\n".join(lines + ['  return 0;', '}']))
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")])
    seen = 0
    for line in subprocess.check_output([str(tmp_path / "abi")], text=True).splitlines():
        cname, field, val = line.split()
        ct = structs[cname]
        assert int(val) == (C.sizeof(ct) if field == "size" else getattr(ct, field).offset), (cname, field)
        seen += 1
    assert seen == sum(len(ct._fields_) + 1 for ct in structs.values())


@pytest.mark.parametrize("over, code", [
    (dict(alibi_slopes=P), UNSUPPORTED), (dict(dtype=_lib.SLM_F32), UNSUPPORTED),
    (dict(head_dim=96), SHAPE), (dict(head_dim=32), SHAPE),
    (dict(n_heads=7), INVALID), (dict(block_size=12), INVALID), (dict(k_stride=(0, 1 << 32)), INVALID),
    (dict(num_splits=257), INVALID), (dict(n_tokens=-1), INVALID),
    (dict(query=None), INVALID), (dict(k_scale=None), INVALID), (dict(v_scale=None), INVALID),
    (dict(out=P + 8), ALIGNMENT), (dict(key_cache=P + 8), ALIGNMENT), (dict(q_stride=(0, 1028)), ALIGNMENT),
    (dict(v_stride=(0, 264)), ALIGNMENT), (dict(k_scale=P + 2), ALIGNMENT),
    (dict(num_splits=3), WORKSPACE), (dict(num_splits=3, workspace=P, workspace_bytes=-1), WORKSPACE),
])
def test_every_refusal_precedes_a_launch(over, code):
    a = _args(**over)
    if over.get("workspace_bytes") == -1:   # one byte short of what the plan reports
        a.workspace_bytes = _plan(a)[1].workspace_bytes - 1
    assert _lib.lib().slm_paged_kv_fp8_attention(C.byref(a), None) == code
    assert _lib.lib().slm_paged_kv_fp8_attention(None, None) == INVALID
    assert _lib.lib().slm_paged_kv_fp8_attention(C.byref(_args(n_tokens=0)), None) == 0   # an empty batch: no-op


def test_the_append_refuses_before_a_launch():
    F = lambda **o: _lib.lib().slm_kv_fp8_append(*[o.get(k, d) for k, d in (   # noqa: E731
        ("slot_ids", P), ("keys", P), ("values", P), ("k_stride", 1536), ("v_stride", 1536), ("k_scale", P),
        ("v_scale", P), ("key_cache", P), ("value_cache", P), ("n_tokens", 4), ("n_kv_heads", 2), ("head_dim", 128),
        ("dtype", _lib.SLM_BF16), ("stream", None))])
    assert F(n_tokens=0) == 0 and F(n_tokens=-1) == INVALID and F(keys=None) == INVALID and F(v_scale=None) == INVALID
    assert F(k_stride=128) == INVALID and F(dtype=_lib.SLM_F32) == UNSUPPORTED and F(head_dim=40) == SHAPE
    assert F(values=P + 8) == ALIGNMENT and F(v_stride=1540) == ALIGNMENT and F(key_cache=P + 4) == ALIGNMENT


@pytest.mark.parametrize("n_tokens, n_heads, n_kv_heads, head_dim, max_kv_len, num_splits", [
    (256, 32, 8, 128, 4096, 0), (32, 32, 8, 128, 4096, 0), (1, 32, 8, 128, 4096, 0), (5, 8, 1, 256, 130, 3),
    (3, 4, 4, 64, 100000, 0), (128, 64, 8, 128, 4096, 0)])
def test_the_plan_reports_the_partial_layout(n_tokens, n_heads, n_kv_heads, head_dim, max_kv_len, num_splits):
    rc, p = _plan(_args(n_tokens, n_heads, n_kv_heads, head_dim, max_kv_len=max_kv_len, num_splits=num_splits))
    assert rc == 0 and 1 <= p.n_splits <= 256 and (num_splits == 0 or p.n_splits == num_splits)
    # o_part [n_tokens, n_heads, n_splits, head_dim] fp32, then ml_part [n_tokens, n_heads, n_splits, 2] fp32
    assert p.workspace_bytes == (n_tokens * n_heads * p.n_splits * (head_dim + 2) * 4 if p.n_splits > 1 else 0)
    group = n_heads // n_kv_heads
    assert p.lanes_per_row == head_dim // 16 and p.heads_per_lane * p.n_chunks == group
    assert p.rows_per_iter == p.waves * 64 // (p.lanes_per_row * p.kv_heads_per_wave)
    assert p.grid == n_tokens * (n_kv_heads // p.kv_heads_per_wave) * p.n_chunks * p.n_splits
    assert p.n_splits == 1 or max_kv_len // p.n_splits >= 128 or num_splits     # >= 128 rows a split


def test_the_torch_helpers_round_trip_all_256_codes():
    codes = torch.arange(256, dtype=torch.uint8).view(2, 128)         # [n_kv_heads = 2, head_dim = 128]
    scale = torch.tensor([0.0123, 2.0])
    x = kernels.dequantize_fp8_kv(codes, scale)
    finite = ~x.isnan()
    assert torch.equal(x[finite], (codes.view(torch.float8_e4m3fn).float() * scale.view(2, 1))[finite])
    back = kernels.quantize_fp8_kv(x, scale).view(torch.uint8)
    assert finite.sum() == 254 and torch.equal(back[finite], codes[finite])
    assert (back[~finite] & 0x7F == 0x7F).all()                        # the two NaN codes stay NaN
    assert kernels.quantize_fp8_kv(torch.tensor([[1e6, -1e6]]), torch.ones(1)).view(torch.uint8).tolist() == [[0x7E, 0xFE]]


def test_the_host_layers_take_the_cache_dtype(monkeypatch):
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape
    from scalellm_amd.layers import KVCache
    from scalellm_amd.model_parallel import ParallelArgs
    kv = KVCache(2, 16, 2, 64, torch.float8_e4m3fn, "cpu", k_scale=torch.tensor([0.5, 2.0]))
    assert kv.key_cache.dtype == torch.uint8 and kv.is_fp8 and kv.v_scale.tolist() == [1.0, 1.0]
    assert not KVCache(2, 16, 2, 64, torch.bfloat16, "cpu").is_fp8
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        LlamaDecodeStep(LlamaShape.tiny(), 8, 16, 16, quant_method="none", kv_cache_dtype="int8", device="cpu")
    with pytest.raises(ValueError, match="kv_cache_dtype"):   # a tensor-parallel rank
        LlamaDecodeStep(LlamaShape.tiny(), 8, 16, 16, ParallelArgs(rank=0, world_size=2), quant_method="none",
                        kv_cache_dtype="fp8", device="cpu")
    monkeypatch.setenv("SLM_DECODE_LANES", "64")              # two lanes asked for
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        LlamaDecodeStep(LlamaShape.tiny(), 8, 16, 16, quant_method="none", kv_cache_dtype="fp8", device="cpu")
