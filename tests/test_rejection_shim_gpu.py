"""The C++ shim's slm::RejectionSampler (slm_rejection_sampler_hip.h) and the Python RejectionSampler
(scalellm_amd/speculative.py) drive the same kernel with the same arguments: bit-identical outputs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _shim():
    from scalellm_amd.cpp_host import load_shim
    return load_shim()


def test_forward_is_bit_identical_on_both_hosts():
    from scalellm_amd.speculative import RejectionSampler
    S = _shim()
    n, k, V = 33, 4, 32000
    g = torch.Generator(device=DEV).manual_seed(3)
    target = (torch.randn(n, k + 1, V, device=DEV, generator=g) * 3).to(torch.bfloat16)
    draft = torch.softmax(target[:, :k].float() + torch.randn(n, k, V, device=DEV, generator=g), -1)
    ids = draft.argmax(-1).int()
    ids[:, 1::2] = torch.randint(0, V, (n, k // 2), device=DEV, generator=g, dtype=torch.int32)
    do = torch.arange(n, device=DEV) % 3 != 0
    seeds = torch.arange(n, dtype=torch.int64, device=DEV) * 31 + 7
    pos = torch.arange(n, dtype=torch.int32, device=DEV) * 5
    bonus = torch.randint(0, V, (n, 1), device=DEV, generator=g, dtype=torch.int32)
    for mask in (False, True):
        py = RejectionSampler(do, True, 3, seeds=seeds, positions=pos).forward(ids, draft, target, bonus, mask)
        cc = S.rejection_sampler_forward(do, True, 3, seeds, pos, ids, draft, target, bonus, mask)
        for name in ("next_tokens", "accepted_lens", "logprobs", "top_logprobs", "top_tokens"):
            assert torch.equal(getattr(py, name), getattr(cc, name)), (mask, name)
    tp = torch.softmax(target[:, :k].float(), -1)
    u = torch.rand(n, k, device=DEV, generator=g)
    a = RejectionSampler.random_sample(ids, draft, tp, u, bonus, True, seeds, pos)
    b = S.rejection_random_sample(ids, draft, tp, u, bonus, True, seeds, pos)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a = RejectionSampler.greedy_sample(ids, tp, bonus, True)
    b = S.rejection_greedy_sample(ids, tp, bonus, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    acc = torch.from_numpy(np.array([[0, 1, 0, 1], [1, 0, 1, 1], [1, 1, 1, 1]], bool))
    assert torch.equal(S.build_accepted_mask(acc), RejectionSampler.build_accepted_mask(acc))
