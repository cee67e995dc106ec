"""CPU tests of the fp8 x fp8 linear boundary (include/slm_hip.h section 25)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from scalellm_amd import _lib, kernels
from scalellm_amd._lib import W8A8LinearArgs

from . import fp8_ref
from . import w8a8_ref as ref

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slm_hip.h")
INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT = -1, -2, -3, -5
DEFER, SILU = _lib.SLM_LINEAR_DEFER_REDUCE, _lib.SLM_LINEAR_SILU_MUL
SYMBOLS = ["slm_w8a8_linear", "slm_w8a8_linear_deferred_splits", "slm_w8a8_linear_plan", "slm_w8a8_quantize_act"]


def test_the_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"SLM_API\s+[\w\s\*]+?\b(slm_w8a8_\w*)\s*\(", src))) == SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r"\sT\s+(slm_w8a8_\w*)", out)) == set(SYMBOLS)
    assert all(getattr(_lib.lib(), n).argtypes is not None for n in SYMBOLS)
    assert all(callable(getattr(kernels, n)) for n in ("quantize_fp8_act", "w8a8_linear", "w8a8_linear_plan"))


def test_the_argument_block_matches_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(slm_w8a8_linear_args));', '  printf("f8_size %zu\\n", sizeof(slm_fp8_linear_args));']
    for fname, _ in W8A8LinearArgs._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(slm_w8a8_linear_args, {fname}));')
    (tmp_path / "abi.c").write_text("\n".join(lines + ['  return 0;', '}']))
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")])
    out = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([str(tmp_path / "abi")], text=True).splitlines())}
    assert out["size"] == C.sizeof(W8A8LinearArgs) and out["a_scale"] == out["f8_size"]   # section 15's block, then one
    for fname, _ in W8A8LinearArgs._fields_:
        assert out[fname] == getattr(W8A8LinearArgs, fname).offset, fname


def test_validation_precedes_any_launch():
    F = lambda g: _lib.lib().slm_w8a8_linear(C.byref(g), None)  # noqa: E731 (address 4096 for every pointer: no launch)
    A = ref.host_args
    assert _lib.lib().slm_w8a8_linear(None, None) == INVALID
    for g in (A(8, 4096 + 16, 4096), A(8, 4096, 4096 + 16), A(8, 4096, 4096 + 32, flags=SILU)):   # K % 32, N % 32, N % 64
        assert F(g) == UNSUPPORTED
    for mut, code in [(dict(a=None), INVALID), (dict(w=None), INVALID), (dict(c=None), INVALID), (dict(lda=4096 - 16), INVALID),
                      (dict(lda=4096 + 8), ALIGNMENT), (dict(a_scale=None, w_scale=None), WORKSPACE)]:   # a split plan
        assert F(A(8, 4096, 4096, **mut)) == code, mut
    g = A(8, 4096, 4096)
    g.workspace, g.workspace_bytes = 4096, ref.host_plan(g)[1].workspace_bytes - 1
    assert g.workspace_bytes > 0 and F(g) == WORKSPACE


@pytest.mark.parametrize("M", [1, 32, 128])
def test_the_plan_is_section_15s_with_no_knob_set(M):
    assert _lib.lib().slm_tuning_clear(None) == 0
    for N, K, flags in ((6144, 4096, 0), (4096, 4096, DEFER), (28672, 4096, 0), (28672, 4096, SILU), (4096, 14336, DEFER)):
        for bits in ref.DTYPES:
            mine, theirs = ref.host_plan(ref.host_args(M, K, N, bits, flags)), fp8_ref.host_plan(fp8_ref.host_args(M, K, N, bits, flags))
            assert mine[0] == theirs[0] == 0 and mine[1].lds_bytes == 2 * 32 * mine[1].row_tiles * 128
            theirs[1].lds_bytes = mine[1].lds_bytes                     # the one field that is the kernel's own
            assert bytes(mine[1]) == bytes(theirs[1]), (M, N, K, flags)


def test_act_quant_is_none_or_fp8():
    from scalellm_amd.decode import LlamaDecodeStep, LlamaShape
    from scalellm_amd.layers import ColumnParallelFp8Linear, RowParallelFp8Linear
    from scalellm_amd.model_parallel import ParallelArgs
    pa = ParallelArgs(rank=0, world_size=1)
    for cls in (ColumnParallelFp8Linear, RowParallelFp8Linear):
        make = lambda q: cls(64, 64, False, cls is RowParallelFp8Linear, pa, torch.bfloat16, "cpu", act_quant=q)  # noqa: E731
        assert make(None).act_quant is None and make("fp8").act_quant == "fp8"
        with pytest.raises(ValueError, match="act_quant"):
            make("mxfp4")
    for quant, act in (("fp8", "mxfp4"), ("mxfp4", "fp8"), ("none", "fp8"), ("fp8", "int8")):
        with pytest.raises(ValueError, match="act_quant"):
            LlamaDecodeStep(LlamaShape.tiny(), 8, 16, 16, quant_method=quant, act_quant=act, device="cpu")
