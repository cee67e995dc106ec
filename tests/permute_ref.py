"""numpy references for the MoE token permutation (include/slm_hip.h section 14) and the token dispatchers
(scalellm_amd/moe.py): both row_id_map forms, the row scatter, the un-permute in float64, the all-to-all plan, and
a simulator that runs dispatch -> combine over every rank of an expert-parallel group without a process group.
Nothing here imports the product code."""
import numpy as np
import torch

from .moe_dense_ref import as64, rounded as rounded16, torch_dtype as torch_dtype16

BITS = ("bf16", "f16", "f32")
MANT_BITS = {"bf16": 7, "f16": 10, "f32": 23}      # explicit mantissa bits
MIN_EXP = {"bf16": -126, "f16": -14, "f32": -126}  # exponent of the smallest normal number


def torch_dtype(bits):
    return torch.float32 if bits == "f32" else torch_dtype16(bits)


def rounded(x, bits):
    """x (numpy, any float type) rounded to the dtype, as a torch tensor of that dtype"""
    if bits == "f32":
        return torch.from_numpy(np.asarray(x, dtype=np.float64).astype(np.float32))
    return rounded16(x, bits)


def ulp(v, bits):
    """the spacing of the dtype's numbers at |v| (float64 array in, float64 array out)"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** MIN_EXP[bits])))
    return 2.0 ** (np.maximum(e, MIN_EXP[bits]) - MANT_BITS[bits])


# ---- maps ------------------------------------------------------------------------------------------------------------
def index_map(ids, n_experts):
    """ids [T, k] -> (row_id_map [k, T] int32, tokens_per_expert [E] int32): rows expert-major, within an expert by
    ascending flat index t * k + j (a stable sort of the flattened ids); ids outside [0, E) get -1 and no row"""
    ids = np.asarray(ids, dtype=np.int64)
    T, k = ids.shape
    flat = ids.reshape(-1)
    valid = (flat >= 0) & (flat < n_experts)
    order = np.argsort(np.where(valid, flat, n_experts), kind="stable")
    order = order[:int(valid.sum())]
    rows = np.full(T * k, -1, dtype=np.int32)
    rows[order] = np.arange(order.size, dtype=np.int32)
    counts = np.bincount(flat[valid], minlength=n_experts).astype(np.int32)
    return np.ascontiguousarray(rows.reshape(T, k).T), counts


def mask_map(mask):
    """mask [T, E] bool -> (row_id_map [E, T] int32, tokens_per_expert [E] int32): rows expert-major, within an
    expert by ascending token"""
    m = np.asarray(mask).astype(bool).T                      # [E, T]
    rows = np.full(m.shape, -1, dtype=np.int32)
    rows[m] = np.arange(int(m.sum()), dtype=np.int32)        # row-major over [E, T]: expert, then token
    return rows, m.sum(1).astype(np.int32)


def ids_to_mask(ids, n_experts):
    ids = np.asarray(ids)
    mask = np.zeros((ids.shape[0], n_experts), dtype=bool)
    for j in range(ids.shape[1]):
        ok = (ids[:, j] >= 0) & (ids[:, j] < n_experts)
        mask[np.nonzero(ok)[0], ids[ok, j]] = True
    return mask


# ---- rows ------------------------------------------------------------------------------------------------------------
def permute_rows(tokens, row_map, permuted):
    """the scatter on any array type: permuted[row_map[m, t]] = tokens[t] for 0 <= row_map[m, t] < rows"""
    out = permuted.copy()
    n_maps, T = row_map.shape
    for m in range(n_maps):
        for t in range(T):
            r = int(row_map[m, t])
            if 0 <= r < out.shape[0]:
                out[r] = tokens[t]
    return out


def unpermute64(permuted64, row_map, probs64, n_rows=None):
    """(sum_m p[t, m] * permuted[row_map[m, t]], sum_m |p * x|) in float64; probs64 None = 1"""
    n_maps, T = row_map.shape
    n_rows = permuted64.shape[0] if n_rows is None else n_rows
    out = np.zeros((T, permuted64.shape[1]))
    mag = np.zeros_like(out)
    for m in range(n_maps):
        for t in range(T):
            r = int(row_map[m, t])
            if 0 <= r < n_rows:
                term = permuted64[r] * (1.0 if probs64 is None else probs64[t, m])
                out[t] += term
                mag[t] += np.abs(term)
    return out, mag


def bit_tokens(T, dim, bits, seed=0):
    """[T, dim] rows of the dtype whose BIT PATTERNS encode (t, d): a wrong source row or a shifted vector shows in
    an integer comparison.  Returned as the integer view (int16 / int32), to be .view()ed to the dtype on the GPU"""
    t = np.arange(T, dtype=np.int64)[:, None]
    d = np.arange(dim, dtype=np.int64)[None, :]
    v = (t * 7919 + d * 31 + seed * 104729 + 1)
    if bits == "f32":
        return torch.from_numpy((v & 0x7fffffff).astype(np.int32))
    return torch.from_numpy((v & 0x7fff).astype(np.int16))


def int_dtype(bits):
    return torch.int32 if bits == "f32" else torch.int16


# ---- routing ---------------------------------------------------------------------------------------------------------
def distinct_ids(rng, T, k, E):
    """k distinct experts per token, in random slot order"""
    return np.stack([rng.permutation(E)[:k] for _ in range(T)]).astype(np.int32).reshape(T, k)


# (name, T, k, E, kind): every T * k around the map kernels' chunk sizes (a wave's walk works through 64 entries at
# a time, the count through 256 per workgroup pass: C - 1, C, C + 1, 2C + 1 of both), one / four / many workgroups
# (4 experts per workgroup), the expert limit, and the special routings
INDEX_CASES = [
    ("t1", 1, 1, 1, "random"), ("t1k8", 1, 8, 256, "distinct"), ("t2", 2, 2, 8, "distinct"),
    ("t16", 16, 4, 64, "distinct"), ("t63", 63, 1, 4, "random"), ("t64", 64, 1, 8, "random"),
    ("t65", 65, 1, 8, "random"), ("t129", 129, 1, 4, "random"), ("t255", 255, 1, 64, "random"),
    ("t256", 64, 4, 8, "distinct"), ("t257", 257, 1, 256, "random"), ("t513", 171, 3, 64, "distinct"),
    ("one_expert", 65, 2, 8, "one"), ("empty_experts", 63, 3, 256, "few"), ("duplicates", 16, 4, 4, "random"),
    ("out_of_range", 65, 3, 8, "foreign"), ("e1024", 16, 8, 1024, "distinct"), ("t257k8", 257, 8, 256, "distinct"),
]


def index_case(name, T, k, E, kind):
    rng = np.random.default_rng(sum(map(ord, name)))
    if kind == "distinct":
        return distinct_ids(rng, T, k, E)
    if kind == "one":
        return np.full((T, k), E - 3, dtype=np.int32)
    if kind == "few":                                   # three live experts, far apart
        return rng.choice(np.array([0, E // 2 + 1, E - 1]), size=(T, k)).astype(np.int32)
    ids = rng.integers(0, E, size=(T, k)).astype(np.int32)   # "random": duplicates within a token happen
    if kind == "foreign":
        ids[rng.random((T, k)) < 0.3] = E
        ids[rng.random((T, k)) < 0.1] = -1
        ids[0, 0] = E + 1000
    return ids


# (name, T, E, k or None): mask cases; k None = an irregular mask (0 .. E experts per token)
MASK_CASES = [
    ("t1", 1, 1, 1), ("t1e256", 1, 256, 8), ("t2", 2, 4, 2), ("t16", 16, 64, 4), ("t63", 63, 8, 3),
    ("t64", 64, 8, 2), ("t65", 65, 4, 1), ("t257", 257, 256, 8), ("irregular", 65, 8, None),
    ("odd_e", 63, 7, 3), ("all", 16, 4, 4), ("none", 16, 8, 0),
]


def mask_case(name, T, E, k):
    rng = np.random.default_rng(sum(map(ord, name)) + 17)
    if k is None:
        return rng.random((T, E)) < 0.3
    if k == 0:
        return np.zeros((T, E), dtype=bool)
    return ids_to_mask(distinct_ids(rng, T, k, E), E)


# ---- the all-to-all plan and the multi-rank simulator ---------------------------------------------------------------
def alltoall_plan(counts, rank):
    """counts [ep, E] -> (input_split_sizes, output_split_sizes, tokens_per_local_expert, order): `order` lists, for
    the rows received by `rank` (rank-major, each rank's rows expert-major), the source position of every row of
    the (expert, rank)-ordered result -- built the reference's way, by splitting into chunks and re-concatenating"""
    counts = np.asarray(counts, dtype=np.int64)
    ep, E = counts.shape
    L = E // ep
    local = counts[:, rank * L:(rank + 1) * L]                       # [ep, L]
    ins = counts[rank].reshape(ep, L).sum(1).tolist()
    outs = local.sum(1).tolist()
    chunks = np.split(np.arange(int(local.sum())), np.cumsum(local.reshape(-1))[:-1])   # (rank, expert) order
    order = np.concatenate([chunks[s * L + l] for l in range(L) for s in range(ep)]) if chunks else np.arange(0)
    return ins, outs, local.sum(0), order.astype(np.int64)


def simulate(ep, n_experts, ids_per_rank, tokens_per_rank, probs_per_rank):
    """dispatch -> identity experts -> combine for every rank of an ep-way group (index form).  Returns
    (rows[r]: what rank r's experts see, sorted by (local expert, source rank), tokens_per_local_expert[r],
     combined[r]: float64 [T_r, dim])"""
    L = n_experts // ep
    maps, sends, counts = [], [], []
    for r in range(ep):
        m, c = index_map(ids_per_rank[r], n_experts)
        maps.append(m)
        counts.append(c)
        sends.append(permute_rows(tokens_per_rank[r], m, np.zeros((int(c.sum()), tokens_per_rank[r].shape[1]))))
    counts = np.stack(counts)
    offs = np.concatenate([np.zeros((ep, 1), dtype=np.int64), np.cumsum(counts, 1)], 1)   # [ep, E + 1]
    rows, tple, back = [], [], [[None] * ep for _ in range(ep)]
    for r in range(ep):
        ins, outs, per_expert, order = alltoall_plan(counts, r)
        recv = np.concatenate([sends[s][offs[s, r * L]:offs[s, (r + 1) * L]] for s in range(ep)])
        assert [sends[r][offs[r, d * L]:offs[r, (d + 1) * L]].shape[0] for d in range(ep)] == ins
        assert recv.shape[0] == sum(outs)
        rows.append(recv[order])
        tple.append(per_expert)
        # combine: undo the reorder, then every source rank gets its slice back
        undone = np.empty_like(rows[r])
        undone[order] = rows[r]
        for s, piece in enumerate(np.split(undone, np.cumsum(outs)[:-1])):
            back[s][r] = piece
    combined = []
    for r in range(ep):
        home = np.concatenate(back[r])
        combined.append(unpermute64(home, maps[r], probs_per_rank[r])[0])
    return rows, tple, combined


# the reference's worked example (alltoall_token_dispatcher.cpp:76-123), restated by hand: 4 ranks, 8 experts, top-2,
# two tokens per rank
REF_TABLE_IDS = [[[0, 4], [2, 5]], [[1, 6], [3, 4]], [[3, 7], [0, 4]], [[1, 7], [2, 5]]]
# tokens t1 .. t8 as the values 1 .. 8; what each rank's experts receive, (expert, rank)-ordered ("sort_by_idx")
REF_TABLE_ROWS = [[1, 6, 3, 7], [2, 8, 4, 5], [1, 4, 6, 2, 8], [3, 5, 7]]
REF_TABLE_PER_LOCAL_EXPERT = [[2, 2], [2, 2], [3, 2], [1, 2]]
# rows before the reorder ("all2all" column): (rank, expert)-ordered
REF_TABLE_RECEIVED = [[1, 3, 6, 7], [2, 4, 5, 8], [1, 2, 4, 6, 8], [3, 5, 7]]
