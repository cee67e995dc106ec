"""numpy oracle of the fused MoE router (include/slm_hip.h section 17): the gate GEMM in float64; the routing is
tests/moe_ref.py's (section 10's oracle), imported, not copied."""
import numpy as np
import torch

from .moe_ref import grouped_topk_sigmoid, topk_softmax  # noqa: F401  (the routing oracle, re-exported)


def as64(t):
    """a torch tensor (any float dtype) -> float64 numpy, exactly"""
    return t.detach().cpu().to(torch.float64).numpy()


def router_logits(x, w):
    """x [T, hidden], w [E, hidden] (float64 arrays of the dtype-rounded inputs) -> logits [T, E] float64"""
    return np.asarray(x, np.float64) @ np.asarray(w, np.float64).T


def logit_bound(x, w):
    """per element: 2 * hidden * 2^-24 * sum_h |x w| -- the worst case of an fp32 sum of `hidden` exact terms in any
    order (each of the hidden - 1 additions errs by at most 2^-24 of a partial sum that |x| . |w| bounds, first
    order), doubled as a guard against an accumulate that is not round-to-nearest."""
    hidden = np.asarray(x).shape[1]
    return 2.0 * hidden * 2.0 ** -24 * (np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(w, np.float64)).T)


def exact_inputs(rng, T, E, hidden, dtype):
    """x in {-2..2} / 4, w in {-1, 0, 1} / 8: every product is a multiple of 1 / 32, every partial sum a multiple of
    1 / 32 below 2^24 / 32, so every summation order gives the same fp32 value"""
    x = torch.from_numpy(rng.integers(-2, 3, size=(T, hidden)) / 4.0).to(dtype)
    w = torch.from_numpy(rng.integers(-1, 2, size=(E, hidden)) / 8.0).to(dtype)
    return x, w


def random_inputs(rng, T, E, hidden, dtype, scale=1.0):
    x = torch.from_numpy(rng.standard_normal((T, hidden))).to(dtype)
    w = torch.from_numpy(rng.standard_normal((E, hidden)) * scale / np.sqrt(hidden)).to(dtype)
    return x, w


# (T, E, hidden, dtype): every axis swept once against the base T 33, E 64, hidden 512, bf16, plus the two corners
BASE = (33, 64, 512, torch.bfloat16)
CASES = sorted({BASE} | {(T, 64, 512, torch.bfloat16) for T in (1, 5, 32, 33, 70)} |
               {(33, E, 512, torch.bfloat16) for E in (8, 64, 256)} |
               {(33, 64, H, torch.bfloat16) for H in (32, 96, 512, 4096)} |
               {(33, 64, 512, torch.float16)} |
               {(1, 256, 4096, torch.bfloat16), (70, 8, 96, torch.bfloat16)}, key=str)

# the grouped sigmoid form of an E: (n_expert_groups, topk_group, topk, scaling_factor)
GROUPED = {8: (4, 2, 2, 1.5), 64: (8, 3, 6, 2.5), 256: (8, 4, 8, 2.5)}
SOFTMAX_TOPK = {8: 2, 64: 6, 256: 8}
