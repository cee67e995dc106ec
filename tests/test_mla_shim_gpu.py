"""The C++ shim's slm::mla_paged_kv / slm::mla_set_kv_cache (slm_mla_hip.h) and kernels.mla_paged_kv /
kernels.mla_set_kv_cache drive the same kernels with the same arguments: bit-identical outputs."""
import shutil

import pytest
import torch

from tests.test_mla_gpu import BF16, DEV, ROPE, _ti, make_case, run

pytestmark = pytest.mark.gpu


def _shim():
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler: the shim cannot be built here")
    from scalellm_amd.cpp_host import load_shim
    return load_shim()  # a build, link or import error of the shim fails the test


@pytest.mark.parametrize("q_lens,kv_lens", [([1] * 4, [300, 31, 64, 1000]), ([1, 60, 7], [500, 260, 7])],
                         ids=["decode", "chunked"])
def test_mla_paged_kv_is_bit_identical_on_both_hosts(q_lens, kv_lens):
    S = _shim()
    c = make_case(17, q_lens, kv_lens, 16, 16, 512, BF16, "randn")
    py = run(c)
    cc = torch.full_like(c["q"], float("nan"))
    S.mla_paged_kv(cc, c["q"], c["kv_cache"], c["q_rope"], c["k_rope_cache"], _ti(c["q_cu"]), _ti(c["kv_cu"]),
                   _ti(c["bt"]), _ti(c["bcu"]), c["block_size"], c["max_q_len"], c["max_kv_len"], c["sm_scale"])
    torch.cuda.synchronize()
    assert not torch.isnan(cc).any()
    assert torch.equal(py.view(torch.int16), cc.view(torch.int16))


def test_mla_set_kv_cache_is_bit_identical_on_both_hosts():
    from scalellm_amd import kernels
    S = _shim()
    g = torch.Generator(device=DEV).manual_seed(2)
    kv = torch.randn(40, 512, device=DEV, generator=g).to(BF16)
    kr = torch.randn(40, ROPE, device=DEV, generator=g).to(BF16)
    slots = torch.randperm(128, device=DEV, generator=g)[:40].int()
    caches = [(torch.zeros(128, 512, dtype=BF16, device=DEV), torch.zeros(128, ROPE, dtype=BF16, device=DEV))
              for _ in range(2)]
    kernels.mla_set_kv_cache(slots, kv, kr, *caches[0])
    S.mla_set_kv_cache(slots, kv, kr, *caches[1])
    torch.cuda.synchronize()
    assert torch.equal(caches[0][0], caches[1][0]) and torch.equal(caches[0][1], caches[1][1])
    assert torch.equal(caches[0][0][slots.long()], kv)
