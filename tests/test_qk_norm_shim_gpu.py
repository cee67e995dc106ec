"""The C++ shim's slm::qk_norm_rope_kv_append (slm_mla_hip.h) drives the same kernel with the same arguments as
kernels.qk_norm_rope_kv_append: bit-identical outputs, both forms."""
import shutil

import numpy as np
import pytest
import torch

from tests import qk_norm_ref as qref
from tests.test_qk_norm_exact_gpu import DEV, _bits, _caches, _canary, _dev, _layout, _table

pytestmark = pytest.mark.gpu


def _shim():
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler: the shim cannot be built here")
    from scalellm_amd.cpp_host import load_shim
    return load_shim()  # a build, link or import error of the shim fails the test


@pytest.mark.parametrize("name", ("d128-h16-t70", "d256-h40-t5"))
def test_qk_norm_rope_kv_append_is_bit_identical_on_both_hosts(name):
    from scalellm_amd import kernels
    S, bits, case = _shim(), "bf16", qref.BY_NAME[name]
    q, k, v, qw, kw = qref.inputs(name, bits)
    p, s = qref.index(name)
    pos, slots, tab = torch.from_numpy(p).to(DEV), torch.from_numpy(s).to(DEV), _table("f32", bits, case.D)
    qwd, kwd = _dev(qw, bits), _dev(kw, bits)
    out = []
    for host in ("py", "cc"):
        qd, kd, vd, _ = _layout(case, q, k, v, bits)
        kc, vc = _caches(case, bits)
        if host == "py":
            kernels.qk_norm_rope_kv_append(qd, kd, vd, qwd, kwd, qref.EPS, pos, tab, True, slot_ids=slots,
                                           key_cache=kc, value_cache=vc)
        else:
            S.qk_norm_rope_kv_append(qd, kd, vd, qwd, kwd, qref.EPS, pos, tab, True, slot_ids=slots, key_cache=kc,
                                     value_cache=vc)
        torch.cuda.synchronize()
        out.append([_bits(t) for t in (qd, kd, kc, vc)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert not (out[1][2] == qref.CANARY).all()
    # the slab form
    slabs = torch.from_numpy(qref.random_slabs(name, 2)).to(DEV)
    out = []
    for host in ("py", "cc"):
        buf = _canary((case.T, qref.n_cols(case)), bits)
        qd, kd, vd = qref.split_row(case, buf)
        kc, vc = _caches(case, bits)
        if host == "py":
            kernels.qk_norm_rope_kv_append(qd, kd, vd, qwd, kwd, qref.EPS, pos, tab, False, slot_ids=slots,
                                           key_cache=kc, value_cache=vc,
                                           partials=kernels.DeferredPartials.from_slabs(slabs))
        else:
            S.qk_norm_rope_kv_append(qd, kd, vd, qwd, kwd, qref.EPS, pos, tab, False, slot_ids=slots, key_cache=kc,
                                     value_cache=vc, partials=slabs)
        torch.cuda.synchronize()
        out.append([_bits(t) for t in (buf, kc, vc)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert not (out[1][0] == qref.CANARY).any()
