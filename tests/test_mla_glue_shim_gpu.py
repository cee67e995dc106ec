"""The C++ shim's slm::mla_rope_append and slm::moe_sum_add (slm_mla_hip.h, slm_moe_hip.h) drive the same kernels with
the same arguments as kernels.mla_rope_append and kernels.moe_sum_add: bit-identical outputs, both forms."""
import shutil

import numpy as np
import pytest
import torch

from tests import mla_glue_ref as mref
from tests.test_mla_glue_exact_gpu import DEV, _bits, _caches, _dev, _layout, _table

pytestmark = pytest.mark.gpu


def _shim():
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler: the shim cannot be built here")
    from scalellm_amd.cpp_host import load_shim
    return load_shim()  # a build, link or import error of the shim fails the test


@pytest.mark.parametrize("name", ("h16-t70", "h0-t1"))
def test_mla_rope_append_is_bit_identical_on_both_hosts(name):
    from scalellm_amd import kernels
    S, bits, case = _shim(), "bf16", mref.BY_NAME[name]
    q, kv_a, w = mref.inputs(name, bits)
    p, s = mref.index(name)
    pos, slots, tab, wd = torch.from_numpy(p).to(DEV), torch.from_numpy(s).to(DEV), _table("f32", bits), _dev(w, bits)
    out = []
    for host in ("py", "cc"):
        qd, kd, _ = _layout(case, q, kv_a, bits)
        kvc, krc = _caches(case, bits)
        if host == "py":
            kernels.mla_rope_append(qd, kd, wd, mref.EPS, pos, tab, True, slots, kvc, krc, case.nope)
        else:
            S.mla_rope_append(qd, kd, wd, mref.EPS, pos, tab, True, slots, kvc, krc, case.nope)
        torch.cuda.synchronize()
        out.append((None if qd is None else _bits(qd), _bits(kvc), _bits(krc)))
    for a, b in zip(*out):
        assert (a is None and b is None) or np.array_equal(a, b)
    assert not (out[1][1] == mref.CANARY).all()
    # the slab form
    slabs = torch.from_numpy(mref.random_slabs(name, 2)).to(DEV)
    out = []
    for host in ("py", "cc"):
        qd = torch.zeros(case.T, case.n_heads, case.nope + mref.ROPE, device=DEV, dtype=torch.bfloat16) \
            if case.n_heads else None
        kvc, krc = _caches(case, bits)
        if host == "py":
            kernels.mla_rope_append(qd, None, wd, mref.EPS, pos, tab, False, slots, kvc, krc, case.nope,
                                    partials=kernels.DeferredPartials.from_slabs(slabs))
        else:
            S.mla_rope_append(qd, None, wd, mref.EPS, pos, tab, False, slots, kvc, krc, case.nope, partials=slabs)
        torch.cuda.synchronize()
        out.append((None if qd is None else _bits(qd), _bits(kvc), _bits(krc)))
    for a, b in zip(*out):
        assert (a is None and b is None) or np.array_equal(a, b)


def test_moe_sum_add_is_bit_identical_on_both_hosts():
    from scalellm_amd import kernels
    S = _shim()
    g = torch.Generator(device=DEV).manual_seed(3)
    inp = torch.randn(33, 6, 2048, device=DEV, dtype=torch.bfloat16, generator=g)
    add = torch.randn(33, 2048, device=DEV, dtype=torch.bfloat16, generator=g)
    a, b = torch.empty_like(add), torch.empty_like(add)
    kernels.moe_sum_add(inp, add, a)
    S.moe_sum_add(inp, add, b)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and not torch.equal(a, add)
