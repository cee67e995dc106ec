"""CPU test of the grouped W4A4 GEMM's boundary (include/slm_hip.h section 23, slm_moe_w4a4_gemm): every argument rule
returns its error code before any launch (address 4096 stands for every pointer and is never dereferenced)."""
import ctypes as C

import pytest

from scalellm_amd import _lib

INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -5
K0, N0 = 256, 128
KB, KS = K0 // 2, K0 // 32        # bytes of a code row, of a scale row
SILU, QUANT = _lib.SLM_MOE_SILU_MUL, _lib.SLM_MOE_QUANT_OUT
QOUT = dict(flags=SILU | QUANT, ldc=N0 // 4)


def _call(**kw):
    g = _lib.MoeW4A4GemmArgs()
    for f in ("a", "a_scale", "w", "w_scale", "c", "c_scale", "sorted_token_idxes", "expert_ids", "n_padded_tokens"):
        setattr(g, f, 4096)
    g.K, g.N = K0, N0
    g.lda, g.ldas, g.ldw, g.lds, g.ldc, g.ldcs = KB, KS, KB, KS, N0, N0 // 64
    g.w_expert_stride, g.w_scale_expert_stride = N0 * KB, N0 * KS
    g.n_flat, g.a_div, g.n_experts, g.max_blocks, g.dtype, g.flags = 8, 2, 4, 4, _lib.SLM_BF16, 0
    for k, v in kw.items():
        setattr(g, k, v)
    return _lib.lib().slm_moe_w4a4_gemm(C.byref(g), None)


@pytest.mark.parametrize("kw,code", [
    # the activation side
    (dict(a_scale=None), INVALID),
    (dict(lda=KB + 8), ALIGNMENT),                                  # lda % 16
    (dict(lda=KB - 16), INVALID),                                   # lda < K / 2
    (dict(ldas=KS - 1), INVALID),
    # the quantised output
    (dict(flags=QUANT, ldc=N0 // 4), INVALID),                      # without SiLU * mul
    (dict(QOUT, row_scale=4096), INVALID),
    (dict(QOUT, c_scale=None), INVALID),
    (dict(QOUT, ldc=N0 // 4 + 8), ALIGNMENT),                       # ldcq % 16
    (dict(QOUT, ldcs=N0 // 64 - 1), INVALID),
    (dict(QOUT, N=96, ldc=32), UNSUPPORTED),                        # (N / 2) % 32
    (dict(flags=8), INVALID),
    (dict(flags=SILU, ldc=64, row_scale=4096), INVALID),
    # T outputs: 8-byte stores
    (dict(c=4096 + 2), ALIGNMENT),
    (dict(ldc=N0 + 2), ALIGNMENT),
    # section 21's weight side
    (dict(w_scale=None), INVALID),
    (dict(ldw=KB - 16), INVALID),
    (dict(w_expert_stride=(N0 - 1) * KB + KB - 16), INVALID),
    (dict(lds=KS - 1), INVALID),
    (dict(w_scale_expert_stride=(N0 - 1) * KS + KS - 1), INVALID),
    (dict(ldw=KB + 8, w_expert_stride=N0 * (KB + 8)), ALIGNMENT),
    (dict(ldw=1 << 25, w_expert_stride=N0 << 25), UNSUPPORTED),     # one expert >= 4 GiB through its stride
    (dict(w_scale=4097, lds=KS + 3, w_scale_expert_stride=N0 * (KS + 3) + 7, w=4096 + 8), ALIGNMENT),   # not the scales
    # shapes, dtype, the list
    (dict(K=144, lda=80, ldw=80), UNSUPPORTED),                     # K % 32
    (dict(dtype=_lib.SLM_F32), UNSUPPORTED),
    (dict(expert_ids=None), INVALID),
    # nothing routed: a no-op, whatever the pointers
    (dict(n_flat=0, a=None, a_scale=None), 0),
    (dict(max_blocks=0, w=None, c=None), 0),
])
def test_moe_w4a4_gemm_validation_precedes_any_launch(kw, code):
    assert _call(**kw) == code
    assert _lib.lib().slm_moe_w4a4_gemm(None, None) == INVALID
