"""What the dense grouped GEMM tests share (include/slm_hip.h section 10, slm_moe_gemm): the fp64 numpy reference
over dtype-rounded inputs, the case lists, and the aligned block list in buffers of a chosen capacity.  The
routing / alignment oracle itself is tests/moe_ref.py."""
import numpy as np
import torch

from . import moe_ref as ref

GEMM_TOL = {"f16": 1e-3, "bf16": 8e-3}      # tests/test_w4_gpu.py: mean relative error of one GEMM on randn inputs
REF_ALLCLOSE = {"f16": 1e-3, "bf16": 1e-2}  # sm80_grouped_gemm_test.cu:177-179, rtol = atol, inputs randn / 10


def torch_dtype(bits):
    return torch.bfloat16 if bits == "bf16" else torch.float16


def rounded(x, bits):
    """x (float64 numpy) rounded once to the dtype, as a CPU tensor of that dtype"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(torch_dtype(bits))


def as64(t):
    return t.detach().cpu().double().numpy()


def allclose(out, want, tol):
    """torch::allclose(out, want, rtol = tol, atol = tol)"""
    return bool(np.all(np.abs(out - want) <= tol + tol * np.abs(want)))


def rel_err(c, r):
    return float(np.abs(c - r).mean() / np.abs(r).mean())


def grouped_ref(a64, w64, ids, a_div):
    """per flat index f = t * k + j:  A[f // a_div] @ W[ids[f]].T  in float64 -> [n_flat, N]"""
    flat = np.asarray(ids).reshape(-1)
    out = np.zeros((flat.size, w64.shape[1]))
    rows = np.arange(flat.size) // a_div
    for e in np.unique(flat):
        sel = np.nonzero(flat == e)[0]
        out[sel] = a64[rows[sel]] @ w64[e].T
    return out


def routing(rng, T, k, E, crowd=False):
    """[T, k] distinct experts per token; crowd: expert 0 takes every token, so T > 32 spills into a second block"""
    if not crowd:
        return np.stack([rng.permutation(E)[:k] for _ in range(T)]).astype(np.int32)
    ids = np.zeros((T, k), np.int32)
    for t in range(T):
        ids[t, 1:] = 1 + rng.permutation(E - 1)[:k - 1]
    return ids


def aligned(ids_np, E, device, blocks=None):
    """the aligned block list of moe_ref in buffers of `blocks` blocks (default: the capacity rule); entries past
    n_padded hold the padding id and expert 0.  Returns (sorted, expert_ids, n_padded) on the device."""
    n_flat = ids_np.size
    cap_blocks = ref.align_capacity(n_flat, E, 32)[1]
    blocks = cap_blocks if blocks is None else blocks
    assert blocks >= cap_blocks
    rs, re_, rn, _ = ref.align_block(ids_np, E, 32)
    srt = np.full(blocks * 32, n_flat, np.int32)
    eid = np.zeros(blocks, np.int32)
    srt[:rn], eid[:rn // 32] = rs, re_
    return (torch.from_numpy(srt).to(device), torch.from_numpy(eid).to(device),
            torch.tensor([rn], dtype=torch.int32, device=device))


# ---- the reference's grid (sm80_grouped_gemm_test.cu:183-192), thinned --------------------------------------------
REF_AXES = ((1, 3, 32, 96), (32, 64, 96, 128), (32, 64, 96, 128), (8, 16, 64), (1, 2, 4))   # m, n, k, E, topk


def ref_cases():
    cases, i = [], 0
    for m in REF_AXES[0]:
        for n in REF_AXES[1]:
            for k in REF_AXES[2]:
                for E in REF_AXES[3]:
                    for topk in REF_AXES[4]:
                        i += 1
                        if i % 11 == 0:                 # 576 / 11: 52 per dtype
                            cases.append((m, n, k, E, topk))
    return cases


REF_CASES = ref_cases()

# ---- the project's grid: ring wrap and odd chunk counts, a part-filled last column tile, a second block ------------
PROJECT_AXES = ((128, 384, 640), (64, 128, 160, 320), (1, 3, 33, 96), ("k", 1))             # K, N, T, a_div
PROJECT_E, PROJECT_TOPK = 8, 2
PROJECT_CASES = [(K, N, T, ad) for K in PROJECT_AXES[0] for N in PROJECT_AXES[1] for T in PROJECT_AXES[2]
                 for ad in PROJECT_AXES[3]]
