"""CPU tests of the grouped W8A8 GEMM boundary (include/slm_hip.h section 26, slm_moe_w8a8_gemm): the symbol, the
struct against the header, and the argument rules that return before any launch."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from scalellm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")
OK, INVALID, UNSUPPORTED, ALIGNMENT = 0, -1, -2, -5
K0, N0, SILU, BIG = 256, 128, _lib.SLM_MOE_SILU_MUL, 1 << 16


def _args(**kw):
    g = _lib.MoeW8A8GemmArgs()
    g.a = g.a_scale = g.w = g.w_scale = g.c = g.sorted_token_idxes = g.expert_ids = g.n_padded_tokens = 4096
    g.K, g.N, g.lda, g.ldw, g.ldc = K0, N0, K0, K0, N0
    g.w_expert_stride, g.w_scale_expert_stride = N0 * K0, N0
    g.n_flat, g.a_div, g.n_experts, g.max_blocks, g.dtype, g.flags = 8, 2, 4, 4, _lib.SLM_BF16, 0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_the_symbol_is_declared_exported_and_bound():
    assert re.search(r"SLM_API\s+int\s+slm_moe_w8a8_gemm\s*\(const slm_moe_w8a8_gemm_args\*", open(HEADER).read())
    fn = _lib.lib().slm_moe_w8a8_gemm
    assert fn.argtypes[0]._type_ is _lib.MoeW8A8GemmArgs and fn(None, None) == INVALID


def test_the_struct_is_section_16s_plus_a_scale(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cls, base = _lib.MoeW8A8GemmArgs, _lib.MoeFp8GemmArgs
    assert cls._fields_[:-1] == base._fields_ and cls.a_scale.offset == C.sizeof(base)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             '  printf("size %zu\\nbase %zu\\n", sizeof(slm_moe_w8a8_gemm_args), sizeof(slm_moe_fp8_gemm_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(slm_moe_w8a8_gemm_args, {f}));' for f, _ in cls._fields_]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines + ['  return 0;', '}']))
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert out.pop("size") == C.sizeof(cls) and out["a_scale"] == out.pop("base")
    assert out == {f: getattr(cls, f).offset for f, _ in cls._fields_}


@pytest.mark.parametrize("want, kw", [
    (INVALID, dict(n_flat=-1)), (INVALID, dict(K=0)), (INVALID, dict(N=-32)), (INVALID, dict(a_div=0)),
    (INVALID, dict(n_experts=0)), (INVALID, dict(max_blocks=-1)),
    (INVALID, dict(a=None)), (INVALID, dict(w=None)), (INVALID, dict(c=None)), (INVALID, dict(sorted_token_idxes=None)),
    (INVALID, dict(expert_ids=None)), (INVALID, dict(n_padded_tokens=None)),
    (INVALID, dict(flags=1)), (INVALID, dict(flags=SILU | 4)),                    # no SLM_MOE_QUANT_OUT here
    (INVALID, dict(flags=SILU, ldc=64, row_scale=4096)),
    (INVALID, dict(lda=240)), (INVALID, dict(ldw=240)), (INVALID, dict(ldc=124)), (INVALID, dict(flags=SILU, ldc=60)),
    (INVALID, dict(w_expert_stride=(N0 - 1) * K0 + 240)), (INVALID, dict(ldw=K0 + 16, w_expert_stride=N0 * K0)),
    (INVALID, dict(w_scale_expert_stride=N0 - 1)),
    (UNSUPPORTED, dict(dtype=_lib.SLM_F32)), (UNSUPPORTED, dict(K=144, lda=144, ldw=144)),
    (UNSUPPORTED, dict(N=112, ldc=112)), (UNSUPPORTED, dict(N=96, ldc=48, flags=SILU)),
    (UNSUPPORTED, dict(K=BIG, N=BIG, lda=BIG, ldw=BIG, ldc=BIG, w_expert_stride=BIG * BIG, w_scale_expert_stride=BIG)),
    (UNSUPPORTED, dict(ldw=1 << 25, w_expert_stride=N0 << 25)), (UNSUPPORTED, dict(n_flat=(1 << 31) - 256)),
    (ALIGNMENT, dict(a=4096 + 8)), (ALIGNMENT, dict(w=4096 + 8)), (ALIGNMENT, dict(lda=K0 + 8)),     # lda: bytes, % 16
    (ALIGNMENT, dict(c=4096 + 4)), (ALIGNMENT, dict(ldc=N0 + 2)),                 # 8-byte stores of C
    (ALIGNMENT, dict(row_scale=4098)), (ALIGNMENT, dict(w_scale=4098)), (ALIGNMENT, dict(a_scale=4098)),
    (ALIGNMENT, dict(ldw=K0 + 8, w_expert_stride=N0 * (K0 + 8))), (ALIGNMENT, dict(w_expert_stride=N0 * K0 + 8)),
    (OK, dict(n_flat=0, a=None, c=None)), (OK, dict(max_blocks=0, w=None, w_scale=None, a_scale=None)),
])
def test_argument_rules_return_before_any_launch(want, kw):
    assert _lib.lib().slm_moe_w8a8_gemm(C.byref(_args(**kw)), None) == want
