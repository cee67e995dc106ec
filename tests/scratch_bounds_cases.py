"""Case table of the scratch-bounds tests: every entry that takes a caller-supplied workspace, run in a buffer of
exactly the size its *_workspace_bytes query reports (tests/test_scratch_bounds_gpu.py), and the host-side checks of
that size against the documented layouts (tests/test_scratch_bounds_cpu.py).  Imports no GPU code.

A case is (name, family, entry, knobs, spec): `entry` is the C-ABI function whose workspace the case exercises,
`knobs` the tuning overrides that select the form, `spec` the family's shape.  The argument blocks built here carry
FAKE addresses (256-aligned, never dereferenced) and serve the host-side queries: plan, split count, workspace size
and the refusal of a short workspace.

The guard layout of one scratch request: [pre-guard PRE_GUARD bytes][region: exactly the reported bytes][post-guard
max(region, POST_MIN) bytes] inside one uint8 allocation; guard_violations() lists the guard bytes that changed.
"""
import ctypes as C
from collections import namedtuple

from tests import attn_exact_cases as AX
from tests import dense_ref, fp8_ref
from tests import w4_exact_cases as WX

FAKE = 1 << 20                    # stands for every pointer of a host-side query
PRE_GUARD = 4096                  # keeps the region 256-byte aligned inside its allocation
POST_MIN = 1 << 20
# the stream-K form's fixed workspace (csrc/w4_common.h): W4_XL_SK_WGS slots of one 256 x 256 fp32 tile, then the
# ticket / flag block that the host clears on every call
XL_SK_SLOT_BYTES = 256 * 256 * 4
XL_SK_SLOTS = 256 * XL_SK_SLOT_BYTES
XL_SK_SYNC = 2048

Case = namedtuple("Case", "name family entry knobs spec")


def round256(n):
    return (n + 255) // 256 * 256


# ---- guards ---------------------------------------------------------------------------------------------------------
def guard_violations(buf, nbytes, byte, pre=PRE_GUARD, limit=8):
    """Offsets (relative to the region's first byte: negative = pre-guard, >= nbytes = post-guard) of up to `limit`
    guard bytes of the uint8 tensor `buf` that differ from `byte`; [] when both guards are intact"""
    import torch
    bad = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    bad[pre:pre + nbytes] = False
    bad &= buf != byte
    idx = torch.nonzero(bad).flatten()[:limit].cpu().tolist()
    return [i - pre for i in idx]


def post_guard_bytes(nbytes):
    return max(nbytes, POST_MIN)


# ---- attention and MLA: the ws=True rows of the exact tables, plus two of this module ---------------------------------
ATTN_WS = [c for c in AX.STREAM + AX.TILE if c.ws]
# pure decode with graph-padding rows: ml_part sits behind o_part at an offset computed from n_tokens, padding
# included; the classic split (no balanced partition: n_tokens != batch) with an empty share and an empty sequence
DECODE_PAD = AX._c("scratch_decode_pad", 1, [5, 64, 129, 700, 0, 33], 8, 2, 128, 16,
                   "split-KV decode with graph-padding rows", pad_rows=3, ws=True, bits=("bf16",))
# far more shares than keys: most shares of every sequence are empty, and the combine must not read their slots
SPLITS64 = AX._c("scratch_splits64", 1, [5, 64, 129, 1], 8, 2, 128, 16, "classic split-KV, 64 shares", num_splits=64,
                 ws=True, bits=("bf16",))
# a forced count above what the combine pass merges: clamped to COMBINE_MAX_SPLITS = 256 (attn.hip) in the plan, the
# workspace and the kernels alike
SPLITS300 = AX._c("scratch_splits300", 1, [5, 700, 129], 8, 2, 128, 16, "classic split-KV, 300 shares asked, 256 given",
                  num_splits=300, splits=256, ws=True, bits=("bf16",))
# every kernel of a tile-kernel call writes partials (tile_splits3_w-1's batch), with graph-padding rows behind it
TILE_PAD = AX._c("scratch_tile_splits3_pad", [65, 40, 5, 1, 17, 2, 1], [300, 200, 65, 200, 129, 2, 0], 16, 8, 128, 16,
                 "tile kernel split-KV, 3 shares, graph-padding rows", pad_rows=3, ws=True, splits=3, bits=("bf16",),
                 SLM_ATTN_TILE_SPLITS=3)
MLA_WS = [c for c in AX.MLA if c.ws] + [
    # the largest split count the entry takes, over two 64-key tiles at most
    AX._c("scratch_mla_s1024", 1, [33, 1, 100], 8, 1, 128, 16, "mla, 1024 splits over 1 / 2 KV tiles", kind="mla",
          num_splits=1024, ws=True, bits=("bf16",)),
    # mla_decode_b5 split three ways, its graph-padding rows kept
    AX._c("scratch_mla_decode_pad_s3", 1, [129, 0, 33, 1, 200], 16, 1, 512, 16, "mla decode, 3 splits, graph padding",
          kind="mla", num_splits=3, pad_rows=2, ws=True, bits=("bf16",))]

CASES = []
for _c in ATTN_WS:
    CASES.append(Case("attn-" + _c.name, "attn", "slm_paged_kv_varlen_mha", dict(_c.knobs), dict(attn=_c, phased=False)))
CASES.append(Case("attn-bal_b20_blk16-phased", "attn", "slm_paged_kv_varlen_mha", dict(AX.BY_NAME["bal_b20_blk16"].knobs),
                  dict(attn=AX.BY_NAME["bal_b20_blk16"], phased=True)))
for _c in (DECODE_PAD, SPLITS64, SPLITS300, TILE_PAD):
    CASES.append(Case("attn-" + _c.name, "attn", "slm_paged_kv_varlen_mha", dict(_c.knobs), dict(attn=_c, phased=False)))
for _c in MLA_WS:
    CASES.append(Case("mla-" + _c.name, "mla", "slm_mla_paged_kv", {}, dict(attn=_c)))


# ---- int4 / int8 GEMMs --------------------------------------------------------------------------------------------------
def _w4(name, kernel, knobs, M, N, K, gs, fmt, act=False, bias=False, bits8=False, consumer=None, split=True):
    """split: the plan must split K (slabs in the workspace); consumer: None, "rms_norm" (a deferred call whose slabs
    rms_norm(partials=) sums) or "gemv_norm" (a deferred GEMV whose slabs the norm prologue of a second deferred GEMV
    reads, that GEMV's own slabs summed by rms_norm)"""
    return Case("w4-" + name, "w4", "slm_w4a16_gemm", dict(knobs),
                dict(kernel=kernel, M=M, N=N, K=K, gs=gs, fmt=fmt, act=act, bias=bias, bits8=bits8, consumer=consumer,
                     split=split))


_SMALL = WX.SMALL[1]
assert _SMALL.knobs["SLM_W4_SPLITK"] == 3
CASES += [
    _w4("ks-split4", "KS", dict(SLM_W4_SPLITK=4), 32, 1024, 4096, 128, "gptq"),
    _w4("small-split3", "SMALL", _SMALL.knobs, 17, 512, 2048, 64, "gptq", bias=True),
    _w4("general-split2", "GENERAL", dict(SLM_W4_SPLITK=2), 64, 512, 1024, 32, "awq"),
    _w4("general-split7", "GENERAL", dict(SLM_W4_KS_MT2=0, SLM_W4_SPLITK=7), 50, 256, 1792, 128, "awq", bias=True),
    _w4("m128-split4", "M128", dict(SLM_W4_M128=1, SLM_W4_SPLITK=4), 96, 1024, 4096, 64, "gptq"),
    # 144 tiles of 6 chunks in ranges of 4: ranges end inside tiles, so partial tiles go through the slots (at
    # XL_SK[0]'s K = 256 every range is one whole tile and the slots stay unused)
    _w4("stream-k", "XL_SK", WX.XL_SK_FORMS[0][1], *WX.XL_SK[3][:5]),
    # act-order: the activation copy alone, and behind the split-K slabs
    # (act-order needs groups: a per-channel g_idx is all zeros in any order, trivial, and carries no perm)
    _w4("act-order", "SMALL", dict(SLM_W4_KS=0, SLM_W4_SPLITK=1), 8, 384, 2048, 128, "gptq", act=True, split=False),
    _w4("act-order-split7", "GENERAL", dict(SLM_W4_KS_MT2=0, SLM_W4_SPLITK=7), 40, 160, 896, 64, "gptq", act=True),
    # 8-bit layer (two int4 planes over 2K packed rows), group 32: the general kernel, one split per 128-row chunk
    _w4("int8-planes", "GENERAL", {}, 48, 128, 512, 32, "gptq", bits8=True),
    # the GEMV splits K over workgroups only when it defers its reduction: its K slices are the slabs
    _w4("gemv-kslices4-deferred", "GEMV", WX.GEMV_DEFERRED["f16"][3], *WX.GEMV_DEFERRED["f16"][:3], 128, "awq",
        consumer="rms_norm"),
    _w4("gemv-deferred", "GEMV", WX.GEMV_DEFERRED["bf16"][3], *WX.GEMV_DEFERRED["bf16"][:3], 128, "awq",
        consumer="rms_norm"),
    _w4("gemv-norm-prologue", "GEMV", {}, 1, 4096, 4096, 128, "awq", consumer="gemv_norm"),
]


# ---- dense and fp8 linears ----------------------------------------------------------------------------------------------
# (M, N, K, rt, nw, split) of test_dense_exact_gpu.test_every_slab_is_the_sum_over_exactly_its_slice and fp8_ref's
DENSE_SLAB_CASES = [(33, 96, 1312, 2, 2, 3), (1, 160, 672, 1, 4, 5), (129, 32, 640, 4, 4, 2), (65, 96, 256, 1, 1, 2),
                    (160, 160, 1312, 2, 4, 5)]


def _lin(fp8, M, N, K, knobs, consumer="rms_norm", split=None, **extra):
    """a split call with bias (reduced into c, shared workspace), then a deferred one without (slabs in the deferred
    buffer) read by `consumer`"""
    entry = "slm_fp8_linear" if fp8 else "slm_linear"
    name = "%s-%s-%dx%dx%d" % ("fp8" if fp8 else "dense", consumer, M, N, K)
    return Case(name, "linear", entry, dict(knobs), dict(fp8=fp8, M=M, N=N, K=K, consumer=consumer, split=split, **extra))


for _m, _n, _k, _rt, _nw, _s in DENSE_SLAB_CASES:
    CASES.append(_lin(False, _m, _n, _k, dense_ref.knobs(_rt, _nw, _s), split=_s))
for _m, _n, _k, _rt, _nw, _s in fp8_ref.SAME_BITS_CASES:
    CASES.append(_lin(True, _m, _n, _k, dense_ref.knobs(_rt, _nw, _s), split=_s))
# one deferred call per slab consumer: T tokens of a fused [q | k | v] (or [q | latent | k_pe]) projection
ROPE_SHAPE = dict(T=7, H=4, HKV=2, D=32)              # N = (H + 2 HKV) D = 256
QKN_SHAPE = dict(T=5, H=4, HKV=2, D=128)              # N = 1024
MLA_PRO_SHAPE = dict(T=5, H=2, NOPE=128, LATENT=512, ROPE=64)   # N = H (NOPE + ROPE) + LATENT + ROPE = 960
CASES += [
    _lin(False, 7, 256, 1024, dict(SLM_LINEAR_SPLITK=3), consumer="rope", split=3),
    _lin(False, 7, 256, 1024, dict(SLM_LINEAR_SPLITK=3), consumer="gemma", split=3),
    _lin(False, 5, 1024, 512, dict(SLM_LINEAR_SPLITK=2), consumer="qk_norm", split=2),
    _lin(True, 5, 960, 512, dict(SLM_LINEAR_SPLITK=4), consumer="mla_prologue", split=4),
]


# ---- sampling, rejection, router ------------------------------------------------------------------------------------------
SAMPLE_VOCAB = 1000
for _entry in ("slm_sample", "slm_logits_process"):
    for _rows, _mu in ((4, 16), (3, 7)):               # n_rows * max_unique * 4 = 256 (no slack) / 84 (172 of slack)
        CASES.append(Case("%s-%dx%d" % (_entry[4:], _rows, _mu), "sampling", _entry, {},
                          dict(n_rows=_rows, max_unique=_mu, vocab=SAMPLE_VOCAB)))
REJECT_VOCAB = 512
for _k in (1, 3, 4):                                   # 4 (k + 1) 16 = 128 / 256 / 320 bytes of records
    for _lp in (False, True):
        CASES.append(Case("rejection-k%d%s" % (_k, "-logprobs" if _lp else ""), "rejection", "slm_rejection_sample", {},
                          dict(n_seqs=4, k=_k, vocab=REJECT_VOCAB, logprobs=_lp)))
CASES.append(Case("moe-router", "router", "slm_moe_router", {}, dict(T=5, E=8, H=256, topk=2)))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# C-ABI workspace query of every entry
WORKSPACE_QUERY = {"slm_paged_kv_varlen_mha": "slm_paged_kv_varlen_mha_workspace_bytes",
                   "slm_mla_paged_kv": "slm_mla_paged_kv_workspace_bytes",
                   "slm_w4a16_gemm": "slm_w4a16_gemm_workspace_bytes",
                   "slm_linear": "slm_linear_workspace_bytes",
                   "slm_fp8_linear": "slm_fp8_linear_workspace_bytes",
                   "slm_sample": "slm_sample_workspace_bytes",
                   "slm_logits_process": "slm_sample_workspace_bytes",
                   "slm_rejection_sample": "slm_rejection_sample_workspace_bytes",
                   "slm_moe_router": "slm_moe_router_workspace_bytes"}


# ---- host-side argument blocks on FAKE addresses ---------------------------------------------------------------------------
def _bf16():
    from scalellm_amd import _lib
    return _lib.SLM_BF16


def attn_n_tokens(c):
    return sum(c.q_lens) + c.pad_rows


def attn_args(c):
    """slm_attn_args of an attention case as kernels.paged_kv_varlen_mha builds it (contiguous q / out, caches
    [slots, kv_heads, head_dim])"""
    from scalellm_amd import _lib
    a = _lib.AttnArgs()
    for f in ("out", "query", "key_cache", "value_cache", "q_cu_lens", "kv_cu_lens", "block_table", "block_cu_lens"):
        setattr(a, f, FAKE)
    H, HKV, D = c.heads, c.kv_heads, c.head_dim
    a.o_stride[0] = a.q_stride[0] = H * D
    a.o_stride[1] = a.q_stride[1] = D
    a.k_stride[0] = a.v_stride[0] = HKV * D
    a.k_stride[1] = a.v_stride[1] = D
    a.dtype = _bf16()
    a.batch_size, a.n_tokens = len(c.q_lens), attn_n_tokens(c)
    a.n_heads, a.n_kv_heads, a.head_dim = H, HKV, D
    a.block_size, a.max_q_len = c.block, max(max(c.q_lens), 1)
    a.max_kv_len = c.max_kv_hint if c.max_kv_hint is not None else max(c.kv_lens)
    a.sm_scale, a.logits_soft_cap, a.sliding_window = AX.sm_scale_of(c), c.softcap, c.window
    a.num_splits = c.num_splits
    a.n_slots = AX.layout(c).n_slots
    a.workspace, a.workspace_bytes = None, 0
    return a


def mla_args(c):
    from scalellm_amd import _lib
    a = _lib.MlaArgs()
    for f in ("out", "q", "q_rope", "kv_cache", "k_rope_cache", "q_cu_lens", "kv_cu_lens", "block_table",
              "block_cu_lens"):
        setattr(a, f, FAKE)
    H, D, R = c.heads, c.head_dim, AX.MLA_ROPE
    a.o_stride[0], a.o_stride[1] = H * D, D
    a.q_stride[0], a.q_stride[1] = H * D, D
    a.q_rope_stride[0], a.q_rope_stride[1] = H * R, R
    a.kv_stride, a.k_rope_stride = D, R
    a.dtype = _bf16()
    a.batch_size, a.n_tokens, a.n_heads, a.head_dim, a.rope_head_dim = len(c.q_lens), attn_n_tokens(c), H, D, R
    a.block_size, a.max_q_len, a.max_kv_len = c.block, max(max(c.q_lens), 1), max(c.kv_lens)
    a.sm_scale, a.num_splits = AX.sm_scale_of(c), c.num_splits
    a.workspace, a.workspace_bytes = None, 0
    return a


def w4_packed_k_group(s):
    """(packed K, packed group size) of a w4 spec: an 8-bit layer is two int4 planes over 2K rows"""
    from scalellm_amd import _lib
    gs = s["K"] if s["gs"] == -1 else s["gs"]
    if s["bits8"]:
        L = _lib.lib()
        return int(L.slm_w8_packed_rows(s["K"])), int(L.slm_w8_packed_group_size(s["K"], gs))
    return s["K"], gs


def w4_has_perm(s):
    """an act-order layer gathers its activation columns through perm; so does every 8-bit layer (the doubled gather
    of its two planes, slm_w8_prepack_weights' perm2): both copy A into the workspace behind the slabs"""
    return s["act"] or s["bits8"]


def w4_args(s, deferred=None):
    """slm_w4_gemm_args as kernels.gptq_gemm builds them; deferred: set SLM_W4_DEFER_REDUCE (default: the calls of
    a consumer case defer, the others do not)"""
    from scalellm_amd import _lib
    g = _lib.W4GemmArgs()
    g.a = g.wq = g.sz = g.c = FAKE
    g.perm = FAKE if w4_has_perm(s) else None
    g.bias = FAKE if s["bias"] else None
    K, gs = w4_packed_k_group(s)
    g.M, g.K, g.N = s["M"], K, s["N"]
    g.lda, g.ldc = s["K"], s["N"]
    g.group_size, g.dtype = gs, _bf16()
    defer = s["consumer"] is not None if deferred is None else deferred
    g.flags = _lib.SLM_W4_DEFER_REDUCE if defer else 0
    g.workspace, g.workspace_bytes = None, 0
    return g


def linear_args(s, deferred):
    """slm_linear_args / slm_fp8_linear_args of the case's reduced call (with bias) or its deferred call (without)"""
    from scalellm_amd import _lib
    ref = fp8_ref if s["fp8"] else dense_ref
    flags = _lib.SLM_LINEAR_DEFER_REDUCE if deferred else 0
    g = ref.host_args(s["M"], s["K"], s["N"], flags=flags, bias=not deferred)
    for f in ("a", "w", "c") + (("w_scale",) if s["fp8"] else ()):
        setattr(g, f, FAKE)
    g.bias = None if deferred else FAKE
    return g


def sampling_args(s, entry):
    """penalties on for every row (frequency, presence, repetition), temperature, top-k / top-p"""
    from scalellm_amd import _lib
    a = _lib.SamplingArgs()
    n, V = s["n_rows"], s["vocab"]
    a.logits, a.logits_stride, a.dtype, a.n_rows, a.vocab, a.max_unique = FAKE, V, _bf16(), n, V, s["max_unique"]
    for f in ("frequency_penalties", "presence_penalties", "repetition_penalties", "temperatures", "top_p", "top_k",
              "unique_ids", "unique_counts", "unique_lens"):
        setattr(a, f, FAKE)
    if entry == "slm_sample":
        a.do_sample = a.seeds = a.next_tokens = a.probs = a.logprobs = FAKE
    else:
        a.processed, a.processed_stride = 2 * FAKE, V
    a.workspace, a.workspace_bytes = None, 0
    return a


def rejection_args(s):
    from scalellm_amd import _lib
    a = _lib.RejectionArgs()
    n, k, V = s["n_seqs"], s["k"], s["vocab"]
    a.n_seqs, a.k, a.vocab, a.dtype = n, k, V, _bf16()
    a.draft_token_ids = a.draft_probs = a.target = a.bonus_token_ids = a.do_sample = a.seeds = FAKE
    a.next_tokens = a.accepted_lens = FAKE
    a.logprobs = FAKE if s["logprobs"] else None
    a.draft_seq_stride, a.draft_row_stride = k * V, V
    a.target_seq_stride, a.target_row_stride = (k + 1) * V, V
    a.workspace, a.workspace_bytes = None, 0
    return a


def workspace_bytes(case):
    """what the entry's query reports for the case (under the case's knobs, which the caller sets): for the linears
    and the GEMMs with a consumer, (reduced call, deferred call)"""
    from scalellm_amd import _lib
    L = _lib.lib()
    s = case.spec
    if case.family == "attn":
        return int(L.slm_paged_kv_varlen_mha_workspace_bytes(C.byref(attn_args(s["attn"]))))
    if case.family == "mla":
        return int(L.slm_mla_paged_kv_workspace_bytes(C.byref(mla_args(s["attn"]))))
    if case.family == "w4":
        return int(L.slm_w4a16_gemm_workspace_bytes(C.byref(w4_args(s))))
    if case.family == "linear":
        q = getattr(L, case.entry + "_workspace_bytes")
        return int(q(C.byref(linear_args(s, False)))), int(q(C.byref(linear_args(s, True))))
    if case.family == "sampling":
        return int(L.slm_sample_workspace_bytes(C.byref(sampling_args(s, case.entry))))
    if case.family == "rejection":
        return int(L.slm_rejection_sample_workspace_bytes(C.byref(rejection_args(s))))
    need = C.c_size_t(0)
    assert L.slm_moe_router_workspace_bytes(s["T"], s["E"], s["H"], _bf16(), C.byref(need)) == 0
    return int(need.value)
