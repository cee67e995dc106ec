"""Multi-head latent attention, the parts that need no GPU: the numpy reference is pinned to the committed C oracle
by an exact identity, the ctypes mirror of slm_mla_args is pinned to the header, and the host-side halves of the
C ABI's section 11 (validation before any launch, workspace sizing, the split heuristic) are checked on dummy
pointers -- the library loads without a device."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests.mla_ref import mla_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "include")
ROPE = 64

SLM_OK, SLM_ERR_INVALID_ARG, SLM_ERR_UNSUPPORTED, SLM_ERR_WORKSPACE, SLM_ERR_ALIGNMENT = 0, -1, -2, -3, -5


def _mixed_case(rng, head_dim, n_heads, block_size=8):
    """batch 3: one decode, one chunked-prefill and one full-prefill sequence; random block ids (may collide)."""
    q_lens, kv_lens = [1, 5, 19], [37, 30, 19]
    q_cu = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    kv_cu = np.concatenate([[0], np.cumsum(kv_lens)]).astype(np.int32)
    n_blocks = [(k + block_size - 1) // block_size for k in kv_lens]
    bcu = np.concatenate([[0], np.cumsum(n_blocks)]).astype(np.int32)
    total_blocks = sum(n_blocks) + 2
    bt = (rng.integers(0, total_blocks, size=sum(n_blocks)) * block_size).astype(np.int32)
    T, S = int(q_cu[-1]), total_blocks * block_size
    f = lambda *shape: rng.random(shape, dtype=np.float32)  # noqa: E731
    return dict(q=f(T, n_heads, head_dim), q_rope=f(T, n_heads, ROPE), kv_cache=f(S, head_dim),
                k_rope_cache=f(S, ROPE), q_cu=q_cu, kv_cu=kv_cu, bt=bt, bcu=bcu, block_size=block_size)


# mla_ref accumulates in fp64, the C oracle in fp32: that is the only difference between the two on this
# construction.  Largest absolute difference measured over the grid below: 1.6e-6 (outputs are averages of values
# in [0, 1), one ulp of fp32 there is 6e-8); the bound is 4x that.
ORACLE_ABS_BOUND = 4 * 1.6e-6


@pytest.mark.parametrize("head_dim,n_heads", list(itertools.product((128, 512), (1, 8))))
def test_mla_ref_equals_the_oracle_on_the_mqa_identity(head_dim, n_heads):
    """MLA == MQA with K = [kv | k_rope], Q = [q | q_rope], V = [kv | 0] (one KV head), output columns [:head_dim]."""
    c = _mixed_case(np.random.default_rng(head_dim + n_heads), head_dim, n_heads)
    sm_scale = 1.0 / np.sqrt(head_dim + ROPE)
    got = mla_ref(c["q"], c["q_rope"], c["kv_cache"], c["k_rope_cache"], c["q_cu"], c["kv_cu"], c["bt"], c["bcu"],
                  c["block_size"], sm_scale)
    Q = np.concatenate([c["q"], c["q_rope"]], axis=-1)
    K = np.concatenate([c["kv_cache"], c["k_rope_cache"]], axis=-1)[:, None, :]
    V = np.concatenate([c["kv_cache"], np.zeros_like(c["k_rope_cache"])], axis=-1)[:, None, :]
    want = oracle.paged_attn(Q, K, V, c["q_cu"], c["kv_cu"], c["bt"], c["bcu"], c["block_size"], sm_scale)
    assert want.shape == (Q.shape[0], n_heads, head_dim + ROPE)
    assert np.all(want[..., head_dim:] == 0)
    diff = float(np.abs(got - want[..., :head_dim]).max())
    print(f"head_dim {head_dim} n_heads {n_heads}: max |mla_ref - oracle| = {diff:.3e}")
    assert diff <= ORACLE_ABS_BOUND


def test_mla_args_match_the_c_header(tmp_path):
    """Size and every field offset of the ctypes MlaArgs equal what gcc makes of include/slm_hip.h."""
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    from scalellm_amd._lib import MlaArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(slm_mla_args));']
    for fname, _ in MlaArgs._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(slm_mla_args, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", HEADER_DIR, str(src), "-o", str(exe)])
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        field, val = line.split()
        want = C.sizeof(MlaArgs) if field == "size" else getattr(MlaArgs, field).offset
        assert int(val) == want, f"slm_mla_args.{field}: C says {val}, ctypes says {want}"
        seen += 1
    assert seen == len(MlaArgs._fields_) + 1


def _valid_args(n_tokens=4, batch=4, n_heads=16, head_dim=512, max_q_len=1, max_kv_len=512, num_splits=1):
    """A valid argument block over dummy (never dereferenced on the host) 16-byte aligned pointers."""
    from scalellm_amd._lib import SLM_BF16, MlaArgs
    a = MlaArgs()
    a.out, a.q, a.q_rope, a.kv_cache, a.k_rope_cache = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    a.o_stride[0], a.o_stride[1] = n_heads * head_dim, head_dim
    a.q_stride[0], a.q_stride[1] = n_heads * head_dim, head_dim
    a.q_rope_stride[0], a.q_rope_stride[1] = n_heads * ROPE, ROPE
    a.kv_stride, a.k_rope_stride = head_dim, ROPE
    a.q_cu_lens, a.kv_cu_lens, a.block_table, a.block_cu_lens = 0x60000, 0x61000, 0x62000, 0x63000
    a.dtype, a.batch_size, a.n_tokens, a.n_heads = SLM_BF16, batch, n_tokens, n_heads
    a.head_dim, a.rope_head_dim, a.block_size = head_dim, ROPE, 64
    a.max_q_len, a.max_kv_len, a.sm_scale = max_q_len, max_kv_len, 1.0 / 24.0
    a.workspace, a.workspace_bytes, a.num_splits = None, 0, num_splits
    return a


def _set(field, value):
    def mutate(a):
        if isinstance(value, tuple):
            getattr(a, field)[value[0]] = value[1]
        else:
            setattr(a, field, value)
    return mutate


def _short_workspace(a):
    from scalellm_amd import _lib
    a.num_splits = 4
    a.workspace = 0x70000
    a.workspace_bytes = _lib.lib().slm_mla_paged_kv_workspace_bytes(C.byref(a)) - 1


MUTATIONS = [
    ("null out", _set("out", None), SLM_ERR_INVALID_ARG),
    ("null q_rope", _set("q_rope", None), SLM_ERR_INVALID_ARG),
    ("null k_rope_cache", _set("k_rope_cache", None), SLM_ERR_INVALID_ARG),
    ("null block_table", _set("block_table", None), SLM_ERR_INVALID_ARG),
    ("block_size 48", _set("block_size", 48), SLM_ERR_INVALID_ARG),
    ("block_size 0", _set("block_size", 0), SLM_ERR_INVALID_ARG),
    ("head_dim 192", _set("head_dim", 192), SLM_ERR_UNSUPPORTED),
    ("head_dim 64", _set("head_dim", 64), SLM_ERR_UNSUPPORTED),
    ("head_dim 0", _set("head_dim", 0), SLM_ERR_UNSUPPORTED),
    ("rope_head_dim 32", _set("rope_head_dim", 32), SLM_ERR_UNSUPPORTED),
    ("dtype f32", _set("dtype", 2), SLM_ERR_UNSUPPORTED),
    ("misaligned q", _set("q", 0x20008), SLM_ERR_ALIGNMENT),
    ("misaligned kv_cache", _set("kv_cache", 0x40002), SLM_ERR_ALIGNMENT),
    ("q token stride", _set("q_stride", (0, 16 * 512 + 4)), SLM_ERR_ALIGNMENT),
    ("q_rope head stride", _set("q_rope_stride", (1, ROPE + 2)), SLM_ERR_ALIGNMENT),
    ("out head stride", _set("o_stride", (1, 512 + 1)), SLM_ERR_ALIGNMENT),
    ("kv slot stride", _set("kv_stride", 512 + 4), SLM_ERR_ALIGNMENT),
    ("missing workspace", _set("num_splits", 4), SLM_ERR_WORKSPACE),
    ("short workspace", _short_workspace, SLM_ERR_WORKSPACE),
]


@pytest.mark.parametrize("what,mutate,status", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_validation_precedes_any_launch(what, mutate, status):
    """Every status of section 11 comes back for its mutation of a valid block -- on a machine without a GPU, over
    pointers no launch could survive."""
    from scalellm_amd import _lib
    a = _valid_args()
    mutate(a)
    assert _lib.lib().slm_mla_paged_kv(C.byref(a), None) == status, what


def test_empty_batch_is_ok_without_a_launch():
    from scalellm_amd import _lib
    L = _lib.lib()
    a = _valid_args()
    a.batch_size = 0
    assert L.slm_mla_paged_kv(C.byref(a), None) == SLM_OK
    a = _valid_args()
    a.n_tokens = 0
    assert L.slm_mla_paged_kv(C.byref(a), None) == SLM_OK
    assert L.slm_mla_set_kv_cache(None, None, None, 512, 64, None, None, 512, 64, 0, 512, 64, 1, None) == SLM_OK
    assert L.slm_mla_set_kv_cache(None, 0x1000, 0x2000, 512, 64, 0x3000, 0x4000, 512, 64, 3, 512, 64, 1,
                                  None) == SLM_ERR_INVALID_ARG
    assert L.slm_mla_set_kv_cache(0x500, 0x1000, 0x2000, 516, 64, 0x3000, 0x4000, 512, 64, 3, 512, 64, 1,
                                  None) == SLM_ERR_ALIGNMENT


def test_workspace_bytes_and_auto_splits_are_pure_host_functions():
    from scalellm_amd import _lib, kernels
    L = _lib.lib()

    def ws(**kw):
        a = _valid_args(**kw)
        return int(L.slm_mla_paged_kv_workspace_bytes(C.byref(a)))

    # a forced split count is honoured: fp32 partials [tokens, heads, splits, head_dim] + (m, l) per partial
    assert ws(num_splits=1) == 0
    for s in (2, 3, 8, 64):
        assert ws(num_splits=s) == 4 * 16 * s * (512 + 2) * 4
    # non-decreasing in splits and in n_tokens x n_heads
    sizes = [ws(num_splits=s) for s in range(1, 20)]
    assert sizes == sorted(sizes)
    sizes = [ws(num_splits=4, n_tokens=t, batch=t) for t in (1, 2, 7, 64, 1000)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    sizes = [ws(num_splits=4, n_heads=h) for h in (1, 8, 16, 24, 128)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    # the heuristic: no split once the batch alone yields at least 256 workgroups (of 32 rows, or 64 once a sequence has more than 32)
    auto = kernels.mla_paged_kv_auto_splits
    assert auto(n_tokens=256, batch_size=256, n_heads=16, head_dim=512, max_q_len=1, max_kv_len=1 << 20) == 1
    assert auto(n_tokens=128, batch_size=128, n_heads=128, head_dim=512, max_q_len=1, max_kv_len=1 << 20) == 1
    assert auto(n_tokens=1024, batch_size=4, n_heads=128, head_dim=512, max_q_len=256, max_kv_len=1 << 20) == 1
    # ... splits a small batch over a long history, and never a short one
    assert auto(n_tokens=1, batch_size=1, n_heads=16, head_dim=512, max_q_len=1, max_kv_len=4096) > 1
    assert auto(n_tokens=1, batch_size=1, n_heads=16, head_dim=512, max_q_len=1, max_kv_len=100) == 1
    # auto (num_splits = 0) sizes the workspace for the split count the heuristic reports
    a = _valid_args(n_tokens=1, batch=1, max_kv_len=4096, num_splits=0)
    s = int(L.slm_mla_paged_kv_auto_splits(C.byref(a)))
    assert int(L.slm_mla_paged_kv_workspace_bytes(C.byref(a))) == 1 * 16 * s * (512 + 2) * 4
