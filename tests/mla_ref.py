"""fp64 numpy reference of multi-head latent attention over a paged latent cache: a restatement of the reference's
mla_varlen_ref / mla_ref (src/kernels/attention/tests/mla_ref.h), which gathers the cache rows through the block
table itself.  Per sequence b and head h:

    S[q, k]      = sm_scale * (q[q, h, :] . kv[k, :] + q_rope[q, h, :] . k_rope[k, :])
    S[q, k]      = -inf  where  k > q + (kv_len_b - q_len_b)
    out[q, h, :] = softmax_k(S[q, :]) . kv[:, :]

Test infrastructure only (the tests feed it the inputs as rounded to the kernel's dtype)."""
import numpy as np


def seq_slots(b, kv_cu_lens, block_table, block_cu_lens, block_size):
    """Cache slots of sequence b's tokens: table[bcu[b] + (i >> log2 bs)] + (i & (bs - 1))."""
    n = int(kv_cu_lens[b + 1]) - int(kv_cu_lens[b])
    i = np.arange(n, dtype=np.int64)
    first = np.asarray(block_table, dtype=np.int64)[int(block_cu_lens[b]) + i // block_size]
    return first + i % block_size


def mla_ref(q, q_rope, kv_cache, k_rope_cache, q_cu_lens, kv_cu_lens, block_table, block_cu_lens, block_size,
            sm_scale):
    """q [T, H, D], q_rope [T, H, R], kv_cache [S, D], k_rope_cache [S, R] -> out [T, H, D] float64.  Rows of q
    past q_cu_lens[-1] (padding) come back as zeros."""
    q = np.asarray(q, dtype=np.float64)
    q_rope = np.asarray(q_rope, dtype=np.float64)
    kvc = np.asarray(kv_cache, dtype=np.float64)
    krc = np.asarray(k_rope_cache, dtype=np.float64)
    T, H, D = q.shape
    out = np.zeros((T, H, D), dtype=np.float64)
    for b in range(len(q_cu_lens) - 1):
        q0, q1 = int(q_cu_lens[b]), int(q_cu_lens[b + 1])
        q_len = q1 - q0
        slots = seq_slots(b, kv_cu_lens, block_table, block_cu_lens, block_size)
        kv_len = len(slots)
        if q_len == 0 or kv_len == 0:
            continue
        kv, kr = kvc[slots], krc[slots]                                   # [kv_len, D], [kv_len, R]
        s = q[q0:q1].reshape(q_len * H, D) @ kv.T + q_rope[q0:q1].reshape(q_len * H, -1) @ kr.T
        s = (s * float(sm_scale)).reshape(q_len, H, kv_len)
        limit = np.arange(q_len)[:, None] + (kv_len - q_len)              # last visible kv index per query token
        s = np.where(np.arange(kv_len)[None, :] <= limit, 0.0, -np.inf)[:, None, :] + s
        m = s.max(axis=-1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)                              # a row that sees nothing: zeros
        p = np.exp(s - m)
        den = p.sum(axis=-1, keepdims=True)
        p = np.divide(p, den, out=np.zeros_like(p), where=den > 0)
        out[q0:q1] = (p.reshape(q_len * H, kv_len) @ kv).reshape(q_len, H, D)
    return out
