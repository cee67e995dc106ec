"""Host-side mirror of the reference's kernel-level operator API for the decode hot path.

Same names, argument order and meaning as the reference's C++ free functions (and its
pybind test surface `scalellm/csrc/kernels.cu`), implemented by calling the C-ABI HIP
library libslm_hip.so (include/slm_hip.h) on torch's CURRENT stream:

  paged_kv_varlen_mha  <- llm::paged_kv_varlen_mha      src/kernels/attention/attn_api.h:12-27
  set_kv_cache         <- llm::kernel::set_kv_cache     src/kernels/kv_cache_kernels.h:6-11
  awq_repack / gptq_repack / gptq_gemm
                       <- marlin::awq_repack / gptq_repack / gptq_gemm
                                                        src/kernels/quantization/marlin.h:17-37
  rms_norm / apply_rotary_pos_emb(+append) / silu_and_mul   

PyTorch is plumbing here (device memory, streams); every op is a HIP kernel of ours.
There is NO fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import contextlib
import threading
import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import SLM_BF16, SLM_F16, AttnArgs, SlmError, W4GemmArgs, check


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return SLM_BF16
    if t.dtype == torch.float16:
        return SLM_F16
    # the reference asserts fp16/bf16 only as well (common/static_dispatch.h:16-27)
    raise SlmError(f"unsupported dtype {t.dtype}: fp16 / bf16 only")


def _require_gpu(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise SlmError("scalellm_amd kernels need GPU tensors (no CPU fallback)")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------
# launch-shape overrides (sweeps / tests that force one kernel): the library reads the SLM_*
# environment once, at first use; afterwards only this explicit setter changes a knob
# (include/slm_hip.h section 0, csrc/tuning.h)
# ---------------------------------------------------------------------------------------
@contextlib.contextmanager
def tuning(**knobs: int):
    """with kernels.tuning(SLM_W4_MT=8, SLM_W4_SPLITK=2): ...   (restores the previous values)"""
    L = _lib.lib()
    saved = {}
    for name, val in knobs.items():
        v, s = C.c_int32(0), C.c_int32(0)
        check(L.slm_tuning_get(name.encode(), C.byref(v), C.byref(s)), f"slm_tuning_get({name})")
        saved[name] = (v.value, s.value)
        if val is None:
            check(L.slm_tuning_clear(name.encode()), f"slm_tuning_clear({name})")
        else:
            check(L.slm_tuning_set(name.encode(), int(val)), f"slm_tuning_set({name})")
    try:
        yield
    finally:
        for name, (v, s) in saved.items():
            if s:
                L.slm_tuning_set(name.encode(), v)
            else:
                L.slm_tuning_clear(name.encode())


def clear_tuning() -> None:
    """Drop every override, including the ones the environment supplied at load time."""
    check(_lib.lib().slm_tuning_clear(None), "slm_tuning_clear")


# ---------------------------------------------------------------------------------------
# workspaces.  One growable scratch buffer per device (split-KV partials, split-K partials,
# act-order activation copy) and a SEPARATE one for deferred split-K partials (a producer ->
# consumer hand-off that no other kernel's scratch may clobber).  Lifetime rule: a buffer that
# was ever handed to a kernel is never released -- hipGraphs captured earlier keep replaying
# against its raw address (the reference captures graphs in ascending batch size, each after
# a warm-up: llm_engine.cpp:79,223, model_runner.cpp:162-175).  Growth retires the old buffer
# (kept alive in _retired) and doubles at least, so the retired total is bounded by the
# final size.  Size it once up front with reserve_workspace() to avoid retirements.
# ---------------------------------------------------------------------------------------
_workspaces = {}
_deferred_ws = {}    # slot 0
_deferred_ws_b = {}  # slot 1: where a GEMM that CONSUMES slot-0 slabs (norm prologue) leaves its own
_retired = []  # buffers replaced by bigger ones: still referenced by graphs captured before
_deferred_gen = {}  # (device, slot) -> generation counter of that deferred-partials buffer
_sampling_ws = {}   # penalised values of sample / logits_process (slm_sample_workspace_bytes)
_rejection_ws = {}  # per-row records of rejection_sample (slm_rejection_sample_workspace_bytes)


# scratch lane of the calling code path (workspace_lane): 0 unless a step runs two streams.  Per THREAD:
# one worker thread per GPU may each be inside its own lane
_lane_tls = threading.local()


def _dev_key(dev: torch.device):
    return (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(),
            getattr(_lane_tls, "lane", 0))


@contextlib.contextmanager
def workspace_lane(lane: int):
    """Scratch buffers are per (device, lane).  Kernels launched on DIFFERENT streams that may run
    concurrently (the two half-batch lanes of decode.LlamaDecodeStep) must not share the split-KV /
    split-K scratch: each stream's launches are issued inside its own lane.  Lane 0 is the default."""
    prev = getattr(_lane_tls, "lane", 0)
    _lane_tls.lane = int(lane)
    try:
        yield
    finally:
        _lane_tls.lane = prev


@contextlib.contextmanager
def shared_chip(on: bool = True):
    """GEMM calls issued inside run NEXT TO another stream's kernels (the two half-batch decode lanes): they carry
    SLM_W4_SHARES_CHIP, so that the plan keeps to launch shapes whose workgroups fit on a CU beside other waves."""
    prev = getattr(_lane_tls, "shared", False)
    _lane_tls.shared = bool(on)
    try:
        yield
    finally:
        _lane_tls.shared = prev


def _chip_flag() -> int:
    return _lib.SLM_W4_SHARES_CHIP if getattr(_lane_tls, "shared", False) else 0


def _grow(table, nbytes: int, dev: torch.device, what: str) -> torch.Tensor:
    key = _dev_key(dev)
    ws = table.get(key)
    if ws is None or ws.numel() < nbytes:
        if torch.cuda.is_current_stream_capturing():
            kw = "sampling_nbytes" if table is _sampling_ws else "rejection_nbytes" if table is _rejection_ws else \
                "deferred_nbytes" if table is _deferred_ws or table is _deferred_ws_b else "nbytes"
            raise SlmError(f"{what} must be reserved before graph capture "
                           f"(need {nbytes} bytes): call reserve_workspace({kw}=...) first")
        size = max(int(nbytes), 1 << 20, 2 * ws.numel() if ws is not None else 0)
        if ws is not None:
            _retired.append(ws)  # never freed: earlier captures still point into it
        ws = torch.empty(size, dtype=torch.uint8, device=dev)
        table[key] = ws
    return ws


def reserve_workspace(nbytes: int, device: Optional[torch.device] = None,
                      deferred_nbytes: int = 0, sampling_nbytes: int = 0,
                      rejection_nbytes: int = 0) -> torch.Tensor:
    """Size the per-device scratch once, before graph capture.  deferred_nbytes sizes BOTH deferred
    split-K slab buffers (slot 0 and slot 1: a GEMM whose norm prologue consumes slot-0 slabs leaves
    its own in slot 1), so a capture needs no warm-up of exactly that path and nothing is retired
    later.  sampling_nbytes sizes the penalised-value scratch of sample / logits_process
    (slm_sample_workspace_bytes: n_rows * max_unique * 4 bytes).  rejection_nbytes sizes the records of
    rejection_sample (slm_rejection_sample_workspace_bytes: n_seqs * (k + 1) * 16 bytes)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    if sampling_nbytes:
        _grow(_sampling_ws, sampling_nbytes, dev, "sampling workspace")
    if rejection_nbytes:
        _grow(_rejection_ws, rejection_nbytes, dev, "rejection workspace")
    if deferred_nbytes:
        _grow(_deferred_ws, deferred_nbytes, dev, "deferred split-K buffer")
        _grow(_deferred_ws_b, deferred_nbytes, dev, "deferred split-K buffer (slot 1)")
    return _grow(_workspaces, nbytes, dev, "workspace")


def retired_workspace_bytes() -> int:
    return sum(t.numel() for t in _retired)


class DeferredPartials:
    """Handle to the fp32 split-K slabs a gptq_gemm(..., defer_reduce=True) left behind, consumed
    by rms_norm(..., partials=handle).  Falsy when the GEMM wrote `c` as usual."""

    __slots__ = ("ptr", "splits", "numel", "key", "generation", "_keep", "slot")

    def __init__(self, ptr=0, splits=0, numel=0, key=None, generation=0, keep=None, slot=0):
        self.ptr, self.splits, self.numel = ptr, splits, numel
        self.key, self.generation, self._keep, self.slot = key, generation, keep, slot

    @classmethod
    def from_slabs(cls, slabs: torch.Tensor) -> "DeferredPartials":
        """Handle over caller-owned fp32 partial sums [splits, M, N] (slot 2: never overwritten by
        this module, so never stale; the caller keeps them alive and unmodified until consumed)."""
        if slabs.dim() != 3 or slabs.dtype != torch.float32 or not slabs.is_contiguous() or \
                not slabs.is_cuda or slabs.size(0) < 1:
            raise SlmError("from_slabs takes a contiguous fp32 [splits, M, N] device tensor")
        return cls(slabs.data_ptr(), slabs.size(0), slabs.size(1) * slabs.size(2),
                   _dev_key(slabs.device), 0, slabs, 2)

    def check(self, dev: torch.device, numel: int, who: str) -> None:
        if self.key != _dev_key(dev) or self.numel != numel:
            raise SlmError(f"{who}: the handle belongs to another device or shape")
        if self.slot != 2 and _deferred_gen.get((self.key, self.slot)) != self.generation:
            raise SlmError(f"{who}: stale handle -- a later deferred GEMM on this device has "
                           "overwritten the slabs")

    def __bool__(self):
        return self.splits > 0

    def __int__(self):
        return self.splits


# ---------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------
def _attn_args(out, query, key_cache, value_cache, q_cu_lens, kv_cu_lens, block_table,
               block_cu_lens, alibi_slopes, block_size, max_q_len, max_kv_len, sm_scale,
               logits_soft_cap, sliding_window, num_splits) -> AttnArgs:
    _require_gpu(out, query, key_cache, value_cache, q_cu_lens, kv_cu_lens, block_table,
                 block_cu_lens, alibi_slopes)
    if query.dim() != 3 or key_cache.dim() != 3 or value_cache.dim() != 3 or out.dim() != 3:
        raise SlmError("query/out must be [n_tokens, n_heads, head_dim]; caches "
                       "[n_slots, n_kv_heads, head_dim]")
    for t in (out, query, key_cache, value_cache):
        if t.stride(-1) != 1:
            raise SlmError("last dimension must be contiguous (attn_api.cpp:38-45)")
    for t in (q_cu_lens, kv_cu_lens, block_table, block_cu_lens):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise SlmError("index tensors must be contiguous int32")
    if key_cache.dtype != query.dtype or value_cache.dtype != query.dtype or out.dtype != query.dtype:
        raise SlmError("out/query/key_cache/value_cache dtypes must match")
    a = AttnArgs()
    a.out, a.query = out.data_ptr(), query.data_ptr()
    a.key_cache, a.value_cache = key_cache.data_ptr(), value_cache.data_ptr()
    a.o_stride[0], a.o_stride[1] = out.stride(0), out.stride(1)
    a.q_stride[0], a.q_stride[1] = query.stride(0), query.stride(1)
    a.k_stride[0], a.k_stride[1] = key_cache.stride(0), key_cache.stride(1)
    a.v_stride[0], a.v_stride[1] = value_cache.stride(0), value_cache.stride(1)
    a.q_cu_lens, a.kv_cu_lens = q_cu_lens.data_ptr(), kv_cu_lens.data_ptr()
    a.block_table, a.block_cu_lens = block_table.data_ptr(), block_cu_lens.data_ptr()
    if alibi_slopes is not None:
        if alibi_slopes.dtype != torch.float32 or not alibi_slopes.is_contiguous():
            raise SlmError("alibi_slopes must be contiguous float32 [n_heads]")
        a.alibi_slopes = alibi_slopes.data_ptr()
    else:
        a.alibi_slopes = None
    a.dtype = _dtype_code(query)
    a.batch_size = q_cu_lens.numel() - 1
    a.n_tokens = query.size(0)
    a.n_heads, a.n_kv_heads, a.head_dim = query.size(1), key_cache.size(1), query.size(2)
    a.block_size, a.max_q_len, a.max_kv_len = int(block_size), int(max_q_len), int(max_kv_len)
    a.sm_scale, a.logits_soft_cap = float(sm_scale), float(logits_soft_cap)
    a.sliding_window = int(sliding_window)
    a.num_splits = int(num_splits)
    a.workspace, a.workspace_bytes = None, 0
    a.n_slots = min(max(key_cache.size(0), value_cache.size(0)), 2 ** 31 - 1)   # block-table entries are int32
    return a


def paged_kv_varlen_mha(
    out: torch.Tensor,            # [n_tokens, n_heads, head_dim]
    query: torch.Tensor,          # [n_tokens, n_heads, head_dim]
    key_cache: torch.Tensor,      # [n_slots, n_kv_heads, head_dim]
    value_cache: torch.Tensor,    # [n_slots, n_kv_heads, head_dim]
    q_cu_lens: torch.Tensor,      # [batch + 1] int32
    kv_cu_lens: torch.Tensor,     # [batch + 1] int32
    block_table: torch.Tensor,    # flattened first-slot ids, int32
    block_cu_lens: torch.Tensor,  # [batch + 1] int32
    alibi_slopes: Optional[torch.Tensor],  # [n_heads] fp32 or None
    block_size: int,
    max_q_len: int,
    max_kv_len: int,
    sm_scale: float,
    logits_soft_cap: float = 0.0,
    sliding_window: int = -1,
    num_splits: int = 0,          # extension: 0 = heuristic, >0 forces the split-KV count
    total_kv_len: int = 0,        # extension: kv_cu_lens[batch] if the HOST knows it (a scheduling hint like
                                  # max_kv_len, slm_attn_args::total_kv_len), 0 = unknown
    phase: int = 0,               # extension: 0 = the whole call, 1 = everything but the split-KV combine pass,
                                  # 2 = the combine pass only (slm_attn_args::phase; 1 then 2 == 0)
) -> None:
    """Mirror of llm::paged_kv_varlen_mha (attn_api.h:12-27): writes `out` in place, async
    on the current stream."""
    L = _lib.lib()
    a = _attn_args(out, query, key_cache, value_cache, q_cu_lens, kv_cu_lens, block_table,
                   block_cu_lens, alibi_slopes, block_size, max_q_len, max_kv_len, sm_scale,
                   logits_soft_cap, sliding_window, num_splits)
    a.total_kv_len = int(total_kv_len) if 0 < int(total_kv_len) < 2 ** 31 else 0
    a.phase = int(phase)
    if a.n_tokens == 0 or a.batch_size == 0:
        return
    need = L.slm_paged_kv_varlen_mha_workspace_bytes(C.byref(a))
    if need:
        ws = reserve_workspace(need, query.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    check(L.slm_paged_kv_varlen_mha(C.byref(a), _stream()), "slm_paged_kv_varlen_mha")


def visible_kv_hint(max_kv_len: int, max_q_len: int, sliding_window: int) -> int:
    """The max_kv_len HINT of a call whose rows all look through a sliding window (paged_kv_varlen_mha's count: the
    keys behind the query; < 0 = none): a pure-decode row streams at most sliding_window + 1 keys however long its
    sequence is, and the plan sizes the KV splits (>= 64 rows a share) from the hint -- given the context length
    instead, a 32 k context cuts a 4 k window into 128 shares where 32 fill the chip (26 vs 19 us at batch 1).
    Like every value of the hint it only shapes the launch."""
    if sliding_window < 0 or max_q_len > 1:
        return int(max_kv_len)
    return min(int(max_kv_len), int(sliding_window) + 1)


_decode_q_cu = {}  # (device key, batch) -> arange(batch + 1) int32: the q_cu_lens of a pure-decode call


def paged_decode_attention(
    out: torch.Tensor,            # [batch, n_heads, head_dim]
    query: torch.Tensor,          # [batch, n_heads, head_dim]: ONE query token per sequence, its last
    key_cache: torch.Tensor,      # [n_slots, n_kv_heads, head_dim]
    value_cache: torch.Tensor,    # [n_slots, n_kv_heads, head_dim]
    kv_cu_lens: torch.Tensor,     # [batch + 1] int32, the query token's own key included
    block_table: torch.Tensor,    # flattened first-slot ids, int32
    block_cu_lens: torch.Tensor,  # [batch + 1] int32
    block_size: int,
    max_kv_len: int,
    sm_scale: Optional[float] = None,   # None: head_dim ** -0.5 (Gemma-2: query_pre_attn_scalar ** -0.5)
    logit_softcap: float = 0.0,         # 0 = off; s = cap * tanh(s / cap) on every scaled score, before the mask
    sliding_window: int = 0,            # <= 0 = off; the token at position L - 1 sees the keys p > L - 1 - window
    num_splits: int = 0,
) -> None:
    """Decode attention in the vocabulary of the model configurations (HuggingFace attn_logit_softcapping,
    sliding_window, query_pre_attn_scalar) over paged_kv_varlen_mha's kernels: the soft cap is the kernel's
    compiled-in score transform, the window narrows every workgroup's KV range on the device (pages in front of
    it are never read), and a KV split that falls outside it leaves an l = 0 partial the combine pass ignores.

    `sliding_window` counts the keys a query sees, ITSELF INCLUDED, as the HuggingFace configurations do;
    paged_kv_varlen_mha's counts the keys behind it, as the reference's handler does: window W here is W - 1
    there.  With both options off this IS paged_kv_varlen_mha(..., max_q_len=1, sm_scale): the same launch."""
    if query.dim() != 3 or kv_cu_lens.numel() != query.size(0) + 1:
        raise SlmError("paged_decode_attention takes one query token per sequence: query [batch, n_heads, "
                       "head_dim], kv_cu_lens [batch + 1]")
    if logit_softcap < 0:
        raise SlmError("logit_softcap must be >= 0 (0 = off)")
    n = query.size(0)
    key = (_dev_key(query.device), n)
    q_cu = _decode_q_cu.get(key)
    if q_cu is None:
        q_cu = _decode_q_cu[key] = torch.arange(n + 1, dtype=torch.int32, device=query.device)
    behind = int(sliding_window) - 1 if sliding_window > 0 else -1
    paged_kv_varlen_mha(out, query, key_cache, value_cache, q_cu, kv_cu_lens, block_table, block_cu_lens, None,
                        block_size, 1, visible_kv_hint(max_kv_len, 1, behind),
                        query.size(2) ** -0.5 if sm_scale is None else sm_scale,
                        logits_soft_cap=float(logit_softcap), sliding_window=behind, num_splits=num_splits)


def paged_kv_varlen_mha_auto_splits(query, key_cache, q_cu_lens, block_size, max_q_len,
                                    max_kv_len) -> int:
    """Split-KV count the library's heuristic picks for these sizes (host-side only)."""
    a = AttnArgs()
    a.dtype = _dtype_code(query)
    a.batch_size = q_cu_lens.numel() - 1
    a.n_tokens = query.size(0)
    a.n_heads, a.n_kv_heads, a.head_dim = query.size(1), key_cache.size(1), query.size(2)
    a.block_size, a.max_q_len, a.max_kv_len = int(block_size), int(max_q_len), int(max_kv_len)
    a.k_stride[0], a.v_stride[0] = key_cache.stride(0), key_cache.stride(0)
    return int(_lib.lib().slm_paged_kv_varlen_mha_auto_splits(C.byref(a)))


def paged_kv_varlen_mha_decode_kernel(n_tokens: int, batch_size: int, n_heads: int, n_kv_heads: int,
                                      head_dim: int, block_size: int, max_q_len: int, max_kv_len: int,
                                      dtype=torch.bfloat16, kv_slot_stride: Optional[int] = None) -> str:
    """Name of the kernel the library's plan gives the q_len = 1 rows of such a call
    (slm_paged_kv_varlen_mha_decode_kernel: current tuning table included; host-side only)."""
    a = AttnArgs()
    a.dtype = _lib.SLM_BF16 if dtype == torch.bfloat16 else _lib.SLM_F16
    a.batch_size, a.n_tokens = int(batch_size), int(n_tokens)
    a.n_heads, a.n_kv_heads, a.head_dim = int(n_heads), int(n_kv_heads), int(head_dim)
    a.block_size, a.max_q_len, a.max_kv_len = int(block_size), int(max_q_len), int(max_kv_len)
    a.k_stride[0] = a.v_stride[0] = int(kv_slot_stride or n_kv_heads * head_dim)
    k = int(_lib.lib().slm_paged_kv_varlen_mha_decode_kernel(C.byref(a)))
    if k < 0:
        raise SlmError("slm_paged_kv_varlen_mha_decode_kernel: invalid attention arguments")
    return "attn_tile_kernel" if k == 1 else "attn_token_kernel"


# ---------------------------------------------------------------------------------------
# KV append
# ---------------------------------------------------------------------------------------
def set_kv_cache(slot_ids: torch.Tensor, keys: torch.Tensor, values: torch.Tensor,
                 key_cache: torch.Tensor, value_cache: torch.Tensor) -> None:
    """Mirror of llm::kernel::set_kv_cache (kv_cache_kernels.h:6-11)."""
    L = _lib.lib()
    _require_gpu(slot_ids, keys, values, key_cache, value_cache)
    if slot_ids.dtype != torch.int32 or not slot_ids.is_contiguous():
        raise SlmError("slot_ids must be contiguous int32")
    # keys/values contiguous in (n_kv_heads, head_dim): kv_cache_kernels.cu:50-51
    for t in (keys, values):
        if t.stride(-1) != 1 or t.stride(-2) != t.size(-1):
            raise SlmError("keys/values must be contiguous in their last two dims")
    if not (key_cache.is_contiguous() and value_cache.is_contiguous()):
        raise SlmError("caches must be contiguous [n_slots, n_kv_heads, head_dim]")
    if slot_ids.numel() != keys.size(0) or keys.size(0) != values.size(0):
        raise SlmError("slot_ids / keys / values token counts differ")
    check(L.slm_set_kv_cache(slot_ids.data_ptr(), keys.data_ptr(), values.data_ptr(),
                             keys.stride(0), values.stride(0), key_cache.data_ptr(),
                             value_cache.data_ptr(), keys.size(0), keys.size(1), keys.size(2),
                             _dtype_code(keys), _stream()), "slm_set_kv_cache")


def decode_advance(positions: torch.Tensor, kv_cu_lens: torch.Tensor, new_cache_slots: torch.Tensor,
                   block_table: torch.Tensor, block_cu_lens: torch.Tensor, block_size: int,
                   overflow_flag: torch.Tensor | None = None) -> None:
    """Device-side input build for the next decode step: in-place update of the
    graph's static int32 inputs, replacing the per-step host rebuild + H2D copies of
    Batch::prepare_model_input (engine/batch.cpp:97-255, model_runner.cpp:194-203) for a steady
    decode batch.  Slot arithmetic = Sequence::kv_cache_slots (request/sequence.cpp:303-317)."""
    L = _lib.lib()
    ts = [positions, kv_cu_lens, new_cache_slots, block_table, block_cu_lens]
    if overflow_flag is not None:
        ts.append(overflow_flag)
    _require_gpu(*ts)
    for t in ts:
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise SlmError("decode_advance: all index tensors must be contiguous int32")
    n = positions.numel()
    if kv_cu_lens.numel() != n + 1 or block_cu_lens.numel() != n + 1 or new_cache_slots.numel() != n:
        raise SlmError("decode_advance: inconsistent batch sizes")
    check(L.slm_decode_advance(positions.data_ptr(), kv_cu_lens.data_ptr(), new_cache_slots.data_ptr(),
                               block_table.data_ptr(), block_cu_lens.data_ptr(), n, block_size,
                               overflow_flag.data_ptr() if overflow_flag is not None else None,
                               _stream()), "slm_decode_advance")


def build_step_inputs(q_lens: torch.Tensor, kv_cached: torch.Tensor, block_table: torch.Tensor,
                      block_cu_lens: torch.Tensor, block_size: int, positions: torch.Tensor,
                      q_cu_lens: torch.Tensor, kv_cu_lens: torch.Tensor, new_cache_slots: torch.Tensor,
                      commit: bool = True, overflow_flag: torch.Tensor | None = None) -> None:
    """Device-side input build for ANY batch (SURVEY 8f f4 beyond steady decode): q_cu_seq_lens,
    kv_cu_seq_lens, positions and new_cache_slots of a step from the per-sequence (new tokens,
    tokens cached) arrays and the persistent block table -- the integer work of
    Batch::prepare_model_input (engine/batch.cpp:97-255) without its per-token host loops and
    the H2D copy of the flattened table.  positions / new_cache_slots may be longer than the step's
    tokens (graph padding rows get position 0, slot 0).  commit: kv_cached += q_lens afterwards
    (Sequence::commit_kv_cache)."""
    L = _lib.lib()
    ts = [q_lens, kv_cached, block_table, block_cu_lens, positions, q_cu_lens, kv_cu_lens, new_cache_slots]
    if overflow_flag is not None:
        ts.append(overflow_flag)
    _require_gpu(*ts)
    for t in ts:
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise SlmError("build_step_inputs: all index tensors must be contiguous int32")
    n = q_lens.numel()
    if kv_cached.numel() != n or block_cu_lens.numel() != n + 1 or q_cu_lens.numel() != n + 1 or \
            kv_cu_lens.numel() != n + 1 or new_cache_slots.numel() != positions.numel():
        raise SlmError("build_step_inputs: inconsistent sizes")
    check(L.slm_build_step_inputs(q_lens.data_ptr(), kv_cached.data_ptr(), block_table.data_ptr(),
                                  block_cu_lens.data_ptr(), n, block_size, positions.numel(), 1 if commit else 0,
                                  positions.data_ptr(), q_cu_lens.data_ptr(), kv_cu_lens.data_ptr(),
                                  new_cache_slots.data_ptr(),
                                  overflow_flag.data_ptr() if overflow_flag is not None else None, _stream()),
          "slm_build_step_inputs")


# ---------------------------------------------------------------------------------------
# int4 (AWQ / GPTQ) prepack + GEMM
# ---------------------------------------------------------------------------------------
class PackedW4:
    """Weights in libslm_hip's MFMA-native int4 layout (see include/slm_hip.h section 3).

    Produced once per layer at load time from the CHECKPOINT tensors, exactly where the
    reference repacks into the Marlin layout on first forward
    (qlinear_awq_marlin_impl.cpp:99-125,232-235; qlinear_gptq_marlin_impl.cpp:41-71,181-184).
    """

    def __init__(self, wq, sz, perm, K, N, group_size, dtype, paired=False, k_src=None):
        self.wq, self.sz, self.perm = wq, sz, perm
        self.K, self.N, self.group_size, self.dtype = K, N, group_size, dtype
        # k_src: width of the activations the GEMM takes.  Equal to K except for a padded
        # act-order shard (gptq_repack with uneven groups), whose packed K is larger
        self.k_src = K if k_src is None else k_src
        # paired: a merged [gate | up] weight whose packed column tiles alternate gate / up
        # (SLM_W4_PAIRED) -- the form gptq_gemm(..., silu_mul=True) needs
        self.paired = paired


def _prepack(fmt: int, qweight, qzeros, scales, perm, K, N, group_size, paired=False) -> PackedW4:
    L = _lib.lib()
    _require_gpu(qweight, qzeros, scales, perm)
    for t in (qweight, qzeros):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise SlmError("qweight / qzeros must be contiguous int32")
    if not scales.is_contiguous():
        raise SlmError("scales must be contiguous [n_groups, N]")
    gs = K if group_size in (-1, 0) else int(group_size)
    if K % gs or tuple(scales.shape) != (K // gs, N) or tuple(qzeros.shape) != (K // gs, N // 8):
        raise SlmError(f"scales/qzeros shapes do not match K={K} N={N} group_size={gs}")
    nb_w, nb_sz = L.slm_w4_packed_weight_bytes(K, N), L.slm_w4_packed_sz_bytes(K, N, gs)
    if nb_w == 0 or nb_sz == 0:
        raise SlmError(f"unsupported int4 shape K={K} N={N} group_size={gs} (need K%64, N%32)")
    wq = torch.empty(nb_w // 4, dtype=torch.int32, device=qweight.device)
    sz = torch.empty(nb_sz // 4, dtype=torch.int32, device=qweight.device)
    if perm is not None and (perm.dtype != torch.int32 or not perm.is_contiguous()):
        raise SlmError("perm must be contiguous int32 [K]")
    if paired:
        if N % 64:
            raise SlmError(f"paired (gate | up) prepack needs N % 64 == 0, got N={N}")
        fmt |= _lib.SLM_W4_PAIRED
    check(L.slm_w4_prepack(fmt, qweight.data_ptr(), qzeros.data_ptr(), scales.data_ptr(),
                           perm.data_ptr() if perm is not None else None, K, N, gs,
                           _dtype_code(scales), wq.data_ptr(), sz.data_ptr(), _stream()),
          "slm_w4_prepack")
    return PackedW4(wq, sz, perm, K, N, gs, scales.dtype, paired)


def awq_repack(qweight: torch.Tensor,  # [K, N/8] int32, AWQ interleave
               qzeros: torch.Tensor,   # [G, N/8] int32, AWQ interleave
               scales: torch.Tensor,   # [G, N] fp16/bf16
               group_size: int, paired: bool = False, bits: int = 4) -> PackedW4:
    """Mirror of marlin::awq_repack (+ the host-side zero/scale permutes of
    qlinear_awq_marlin_impl.cpp:34-125), from the AWQ checkpoint format.

    paired: the tensors are a merged [gate | up] weight (multi_parallel_linear.cpp:14-41); pack
    the two halves interleaved by 32-column tile so the GEMM can fuse SiLU*mul (silu_mul=True).
    bits = 8: qweight [K, N/4], qzeros [G, N/4] (byte order [0,2,1,3]); packed as two int4 planes
    (include/slm_hip.h section 3b)."""
    if bits == 8:
        K, N = qweight.size(0), qweight.size(1) * 4
        return _prepack8(_lib.SLM_W8_AWQ, qweight, qzeros, scales, None, K, N, group_size, paired)
    if bits != 4:
        raise SlmError(f"awq_repack: bits must be 4 or 8, got {bits}")
    K, N = qweight.size(0), qweight.size(1) * 8
    return _prepack(_lib.SLM_W4_AWQ, qweight, qzeros, scales, None, K, N, group_size, paired)


def _prepack8(fmt: int, qweight, qzeros, scales, perm, K, N, group_size, paired=False) -> PackedW4:
    """8-bit checkpoint -> two int4 planes over 2K packed rows + the doubled activation gather
    (csrc/w8_planes.hip).  qzeros may be None (symmetric, zero = 128)."""
    L = _lib.lib()
    _require_gpu(qweight, qzeros, scales, perm)
    for t in (qweight, qzeros):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise SlmError("qweight / qzeros must be contiguous int32")
    if not scales.is_contiguous():
        raise SlmError("scales must be contiguous [n_groups, N]")
    gs = K if group_size in (-1, 0) else int(group_size)
    if K % gs or tuple(scales.shape) != (K // gs, N) or \
            (qzeros is not None and tuple(qzeros.shape) != (K // gs, N // 4)):
        raise SlmError(f"scales/qzeros shapes do not match K={K} N={N} group_size={gs} (8-bit)")
    gp = L.slm_w8_packed_group_size(K, gs)
    K2 = L.slm_w8_packed_rows(K)
    nb_w = L.slm_w4_packed_weight_bytes(K2, N)
    nb_sz = L.slm_w4_packed_sz_bytes(K2, N, gp) if gp > 0 else 0
    if gp <= 0 or nb_w == 0 or nb_sz == 0:
        raise SlmError(f"unsupported 8-bit shape K={K} N={N} group_size={gs} (need K%64, N%32, "
                       f"group 32 / 64 / a multiple of 128)")
    if perm is not None and (perm.dtype != torch.int32 or not perm.is_contiguous()):
        raise SlmError("perm must be contiguous int32 [K]")
    if paired:
        if N % 64:
            raise SlmError(f"paired (gate | up) prepack needs N % 64 == 0, got N={N}")
        fmt |= _lib.SLM_W4_PAIRED
    dev = qweight.device
    wq = torch.empty(nb_w // 4, dtype=torch.int32, device=dev)
    sz = torch.empty(nb_sz // 4, dtype=torch.int32, device=dev)
    perm2 = torch.empty(K2, dtype=torch.int32, device=dev)
    check(L.slm_w8_prepack_weights(fmt, qweight.data_ptr(), perm.data_ptr() if perm is not None else None,
                                   K, N, wq.data_ptr(), perm2.data_ptr(), _stream()), "slm_w8_prepack_weights")
    check(L.slm_w8_prepack_sz(fmt, qzeros.data_ptr() if qzeros is not None else None, scales.data_ptr(),
                              K, N, gs, _dtype_code(scales), sz.data_ptr(), _stream()), "slm_w8_prepack_sz")
    return PackedW4(wq, sz, perm2, K2, N, gp, scales.dtype, paired, k_src=K)


def gptq_repack(qweight: torch.Tensor,  # [K/8, N] int32
                qzeros: torch.Tensor,   # [G, N/8] int32 (zero = stored + 1)
                scales: torch.Tensor,   # [G, N]
                group_size: int,
                g_idx: Optional[torch.Tensor] = None, paired: bool = False, bits: int = 4) -> PackedW4:
    """Mirror of marlin::gptq_repack (+ qlinear_gptq_marlin_impl.cpp:41-71): act-order
    checkpoints (g_idx not monotone) are handled like the reference: rows sorted by group
    (perm = argsort(g_idx)), the activation columns gathered by the same perm at GEMM time.
    bits = 8: qweight [K/4, N], qzeros [G, N/4] (or None: symmetric); two int4 planes (slm_hip.h 3b)."""
    if bits not in (4, 8):
        raise SlmError(f"gptq_repack: bits must be 4 or 8, got {bits}")
    K, N = qweight.size(0) * (32 // bits), qweight.size(1)
    gs = K if group_size in (-1, 0) else int(group_size)
    perm = None
    if g_idx is not None and g_idx.numel() > 0:
        if g_idx.numel() != K:
            raise SlmError("g_idx must have K entries")
        trivial = torch.arange(K, device=g_idx.device, dtype=torch.int64) // gs
        if not torch.equal(g_idx.to(torch.int64), trivial):
            perm64 = torch.argsort(g_idx.to(torch.int64), stable=True)
            if not torch.equal(g_idx.to(torch.int64)[perm64], trivial):
                # uneven groups after sorting: a row-parallel shard of an act-order checkpoint
                # (sharded qweight / g_idx, FULL scales: qlinear_gptq_marlin_impl.cpp:236-243,270-276;
                # the reference then runs Marlin with is_k_full = false, :319)
                if bits != 4:
                    raise SlmError("act-order shards with uneven groups are supported for 4-bit weights only")
                return _prepack_uneven_groups(qweight, qzeros, scales, g_idx.to(torch.int64), perm64,
                                              K, N, gs, paired)
            perm = perm64.to(torch.int32).contiguous()
    if bits == 8:
        return _prepack8(_lib.SLM_W8_GPTQ, qweight, qzeros, scales, perm, K, N, gs, paired)
    return _prepack(_lib.SLM_W4_GPTQ, qweight, qzeros, scales, perm, K, N, gs, paired)


_UNEVEN_BLOCK = 32  # smallest scale-group the kernels support: padding granule of an uneven shard


def plan_uneven_groups(g_idx: torch.Tensor, perm: torch.Tensor, n_groups: int):
    """Padded row order of an act-order shard whose groups hold uneven numbers of rows.

    g_idx [K] int64: group of every checkpoint row of the shard (indices into the FULL scale
    table); perm = argsort(g_idx, stable).  The sorted rows of every group are padded up to a
    multiple of 32 rows and the total up to a multiple of 128, so that in the padded order every
    32-row block belongs to exactly one group -- which the kernels handle as group_size = 32 with
    one scale row per block.  Returns (perm_p [Kp] int32: padded position -> checkpoint row, -1 =
    padding; block_group [Kp / 32] int64)."""
    B = _UNEVEN_BLOCK
    dev = g_idx.device
    gs_sorted = g_idx[perm]
    counts = torch.bincount(gs_sorted, minlength=n_groups)
    padded = (counts + B - 1) // B * B
    starts = torch.cumsum(padded, 0) - padded    # first padded position of every group
    cstarts = torch.cumsum(counts, 0) - counts   # first sorted position of every group
    pos = starts[gs_sorted] + (torch.arange(g_idx.numel(), device=dev) - cstarts[gs_sorted])
    total = int(padded.sum().item())
    kp = (total + 127) // 128 * 128
    perm_p = torch.full((kp,), -1, dtype=torch.int32, device=dev)
    perm_p[pos] = perm.to(torch.int32)
    block_group = torch.repeat_interleave(torch.arange(n_groups, device=dev), padded // B)
    if kp > total:  # tail blocks: all padding, any scale row will do
        block_group = torch.cat([block_group, block_group.new_zeros((kp - total) // B)])
    return perm_p.contiguous(), block_group


def _prepack_uneven_groups(qweight, qzeros, scales, g_idx, perm64, K, N, gs, paired) -> PackedW4:
    L = _lib.lib()
    _require_gpu(qweight, qzeros, scales)
    G = scales.size(0)
    if int(g_idx.max().item()) >= G or int(g_idx.min().item()) < 0:
        raise SlmError("g_idx refers to a scale group the scales tensor does not have")
    if tuple(qzeros.shape) != (G, N // 8) or scales.size(1) != N or not scales.is_contiguous():
        raise SlmError(f"scales/qzeros shapes do not match n_groups={G} N={N}")
    perm_p, block_group = plan_uneven_groups(g_idx, perm64, G)
    kp = perm_p.numel()
    fmt = _lib.SLM_W4_GPTQ
    if paired:
        if N % 64:
            raise SlmError(f"paired (gate | up) prepack needs N % 64 == 0, got N={N}")
        fmt |= _lib.SLM_W4_PAIRED
    nb_w = L.slm_w4_packed_weight_bytes(kp, N)
    if nb_w == 0:
        raise SlmError(f"unsupported int4 shape K={kp} N={N}")
    wq = torch.empty(nb_w // 4, dtype=torch.int32, device=qweight.device)
    check(L.slm_w4_prepack_weights(fmt, qweight.data_ptr(), perm_p.data_ptr(), kp, N, wq.data_ptr(),
                                   _stream()), "slm_w4_prepack_weights")
    # fused {scale, magic + zero} rows of the FULL table, then one row per 32-row block
    sz_full = torch.empty(G * N, dtype=torch.int32, device=qweight.device)
    check(L.slm_w4_prepack_sz(fmt, qzeros.data_ptr(), scales.data_ptr(), G * gs, N, gs,
                              _dtype_code(scales), sz_full.data_ptr(), _stream()), "slm_w4_prepack_sz")
    sz = sz_full.view(G, N)[block_group].contiguous().view(-1)
    return PackedW4(wq, sz, perm_p, kp, N, _UNEVEN_BLOCK, scales.dtype, paired, k_src=K)


def _gemm_args(a, packed: PackedW4, c, bias, silu_mul=False) -> W4GemmArgs:
    _require_gpu(a, c, bias)
    if a.dim() != 2 or c.dim() != 2 or a.stride(1) != 1 or c.stride(1) != 1:
        raise SlmError("A [M, K] and C [M, N] must be 2-D with contiguous rows")
    if silu_mul and not packed.paired:
        raise SlmError("silu_mul=True needs weights packed with paired=True (gate | up tiles interleaved)")
    n_out = packed.N // 2 if silu_mul else packed.N
    if a.size(1) != packed.k_src or c.size(1) != n_out or a.size(0) != c.size(0):
        raise SlmError("GEMM shape mismatch")
    if a.dtype != packed.dtype or c.dtype != packed.dtype:
        raise SlmError("activation / output dtype must match the prepacked scales dtype")
    g = W4GemmArgs()
    g.a, g.wq, g.sz = a.data_ptr(), packed.wq.data_ptr(), packed.sz.data_ptr()
    g.perm = packed.perm.data_ptr() if packed.perm is not None else None
    g.bias = bias.data_ptr() if bias is not None else None
    g.c = c.data_ptr()
    g.M, g.K, g.N = a.size(0), packed.K, packed.N
    g.lda, g.ldc = a.stride(0), c.stride(0)
    g.group_size = packed.group_size
    g.dtype = _dtype_code(a)
    g.workspace, g.workspace_bytes = None, 0
    return g


class NormPrologue:
    """RMSNorm computed inside the M <= 4 GEMV (struct slm_w4_norm_prologue): the activations of
    gptq_gemm(x, ..., norm=NormPrologue(...)) are rms_norm(x + residual) * weight, where `x` is the
    tensor passed as `a` -- or, with `partials`, the unwritten output of the deferred GEMM that
    returned the handle.  residual_out receives T(x + residual) and may NOT alias residual or x
    (every workgroup recomputes the sum while one of them stores it)."""

    __slots__ = ("weight", "eps", "residual", "residual_out", "partials", "normed_out")

    def __init__(self, weight: torch.Tensor, eps: float, residual: Optional[torch.Tensor] = None,
                 residual_out: Optional[torch.Tensor] = None,
                 partials: Optional[DeferredPartials] = None,
                 normed_out: Optional[torch.Tensor] = None):
        self.weight, self.eps, self.residual, self.residual_out = weight, eps, residual, residual_out
        self.partials, self.normed_out = partials, normed_out


def gemv_norm_supported(n_tokens: int, packed: PackedW4, dtype: torch.dtype,
                        silu_mul: bool = False, defer_reduce: bool = False) -> bool:
    """Would gptq_gemm(..., norm=...) be accepted for this shape (slm_w4a16_gemv_norm_supported)?"""
    if n_tokens <= 0 or packed.perm is not None or dtype != packed.dtype:
        return False
    g = W4GemmArgs()
    g.a, g.wq, g.sz = None, packed.wq.data_ptr(), packed.sz.data_ptr()
    g.perm, g.bias, g.c = None, None, None
    g.M, g.K, g.N = n_tokens, packed.K, packed.N
    g.lda, g.ldc = packed.K, packed.N // 2 if silu_mul else packed.N
    g.group_size = packed.group_size
    g.dtype = SLM_BF16 if dtype == torch.bfloat16 else SLM_F16
    g.flags = _lib.SLM_W4_SILU_MUL if silu_mul else (_lib.SLM_W4_DEFER_REDUCE if defer_reduce else 0)
    g.workspace, g.workspace_bytes = None, 0
    return bool(_lib.lib().slm_w4a16_gemv_norm_supported(C.byref(g)))


def _set_gemm_flags(g: W4GemmArgs, defer_reduce: bool, silu_mul: bool) -> int:
    """g.flags of a gptq_gemm call; returns the slab count when the call defers its reduction, else 0"""
    chip = _chip_flag()
    g.flags = chip
    if silu_mul:
        g.flags = _lib.SLM_W4_SILU_MUL | chip
    deferred = 0
    if defer_reduce:
        g.flags = _lib.SLM_W4_DEFER_REDUCE | chip
        deferred = _lib.lib().slm_w4a16_gemm_deferred_splits(C.byref(g))
        if not deferred:
            g.flags = chip
    return deferred


def w4_plan(a: torch.Tensor, packed: PackedW4, c: torch.Tensor, bias: Optional[torch.Tensor] = None,
            defer_reduce: bool = False, silu_mul: bool = False) -> "_lib.W4PlanInfo":
    """The launch gptq_gemm would give these very arguments now -- under the tuning knobs and the
    shared_chip() state in force (slm_w4a16_gemm_plan): .kernel_name, grid, kernel-specific variant.
    A host-side query: nothing runs on the GPU."""
    g = _gemm_args(a, packed, c, bias, silu_mul)
    _set_gemm_flags(g, defer_reduce, silu_mul)
    info = _lib.W4PlanInfo()
    check(_lib.lib().slm_w4a16_gemm_plan(C.byref(g), C.byref(info)), "slm_w4a16_gemm_plan")
    return info


def gptq_gemm(a: torch.Tensor, packed: PackedW4, c: torch.Tensor,
              bias: Optional[torch.Tensor] = None, defer_reduce: bool = False,
              silu_mul: bool = False, norm: Optional[NormPrologue] = None) -> DeferredPartials:
    """Mirror of marlin::gptq_gemm (marlin.h:17-25): C[M,N] = A[M,K] . dequant(W) (+ bias),
    fp32 accumulate, written into the pre-allocated `c`.  AWQ and GPTQ share it, as in the
    reference (has_zp true/false): zero points live in the prepacked scale/zero table.

    defer_reduce: when the call is split over K, leave the fp32 partial sums in a dedicated
    device buffer for the consumer (rms_norm(..., partials=handle)) instead of reducing them into
    `c`.  Returns a DeferredPartials handle: truthy (int(handle) = slab count >= 2) when slabs
    were left behind and `c` was NOT written, falsy when `c` was written as usual.

    silu_mul: `packed` is a paired (gate | up) weight and `c` is [M, N/2]: the epilogue applies
    kernel::act_and_mul (activation_kernels.cu:84) -- c = silu(gate) * up, bit-identical to the
    unfused GEMM followed by silu_mul().

    norm: the activations are rms_norm(a + norm.residual) * norm.weight, computed in the GEMV's
    prologue (M <= 4 only: ask gemv_norm_supported first) -- bit-identical to rms_norm() followed
    by this call, two launches less per decoder layer at batch 1."""
    L = _lib.lib()
    if silu_mul and defer_reduce:
        raise SlmError("silu_mul and defer_reduce cannot be combined")
    g = _gemm_args(a, packed, c, bias, silu_mul)
    if g.M == 0:
        return DeferredPartials()
    npro, slot = None, 0
    if norm is not None:
        _require_gpu(norm.weight, norm.residual, norm.residual_out, norm.normed_out)
        for t in (a, norm.weight, norm.residual, norm.residual_out, norm.normed_out):
            if t is not None and (not t.is_contiguous() or t.dtype != a.dtype):
                raise SlmError("norm prologue tensors must be contiguous and of the activation dtype")
        for t in (norm.residual, norm.residual_out, norm.normed_out):
            if t is not None and t.shape != a.shape:
                raise SlmError("norm prologue: residual / residual_out / normed_out must be [M, K]")
        if norm.weight.numel() != packed.K:
            raise SlmError("norm prologue: weight must have K entries")
        if norm.residual is not None and norm.residual_out is None:
            raise SlmError("norm prologue: residual needs a separate residual_out buffer")
        npro = _lib.W4NormPrologue()
        npro.x, npro.partials, npro.n_splits = a.data_ptr(), None, 0
        if norm.partials:
            if not isinstance(norm.partials, DeferredPartials):
                raise SlmError("norm.partials takes the handle gptq_gemm(defer_reduce=True) returned")
            norm.partials.check(a.device, a.numel(), "norm prologue")
            npro.x, npro.partials, npro.n_splits = None, norm.partials.ptr, norm.partials.splits
            slot = 1 if norm.partials.slot == 0 else 0  # its own slabs must not land on the ones it reads
        npro.eps = float(norm.eps)
        npro.residual_in = norm.residual.data_ptr() if norm.residual is not None else None
        npro.residual_out = norm.residual_out.data_ptr() if norm.residual_out is not None else None
        npro.weight = norm.weight.data_ptr()
        npro.normed_out = norm.normed_out.data_ptr() if norm.normed_out is not None else None
    deferred = _set_gemm_flags(g, defer_reduce, silu_mul)
    need = L.slm_w4a16_gemm_workspace_bytes(C.byref(g))
    ws = None
    if need:
        # deferred slabs live in their own buffer: attention split-KV scratch, other split-K GEMMs
        # and act-order copies (which all use the shared workspace) can never overwrite them
        ws = _grow(_deferred_ws_b if slot else _deferred_ws, need, a.device,
                   "deferred split-K buffer") if deferred else reserve_workspace(need, a.device)
        g.workspace, g.workspace_bytes = ws.data_ptr(), ws.numel()
    if npro is not None:
        check(L.slm_w4a16_gemv_norm(C.byref(g), C.byref(npro), _stream()), "slm_w4a16_gemv_norm")
    else:
        check(L.slm_w4a16_gemm(C.byref(g), _stream()), "slm_w4a16_gemm")
    if deferred:
        key = _dev_key(a.device)
        gen = _deferred_gen.get((key, slot), 0) + 1
        _deferred_gen[(key, slot)] = gen  # any older handle on this buffer is now stale
        return DeferredPartials(g.workspace, deferred, g.M * g.N, key, gen, ws, slot)
    return DeferredPartials()


def w4_dequant(packed: PackedW4) -> torch.Tensor:
    """Dense [K, N] weights from the packed form (debug / parity; same dequant code as the GEMM)."""
    L = _lib.lib()
    w = torch.empty(packed.K, packed.N, dtype=packed.dtype, device=packed.wq.device)
    check(L.slm_w4_dequant(packed.wq.data_ptr(), packed.sz.data_ptr(), packed.K, packed.N,
                           packed.group_size, SLM_BF16 if packed.dtype == torch.bfloat16 else SLM_F16,
                           w.data_ptr(), _stream()), "slm_w4_dequant")
    return w


# ---------------------------------------------------------------------------------------
# dense (unquantised) linear: slm_hip.h section 13
# ---------------------------------------------------------------------------------------
def _linear_args(a, weight, w_scale, c, bias, defer_reduce: bool, silu_mul: bool, fp8: bool = False):
    """Checks and argument block of linear() and its plan query, or with fp8 of fp8_linear(): the same block plus
    w_scale, over e4m3 bytes (`weight`) that do not share the activations' dtype"""
    name = "fp8_linear" if fp8 else "linear"
    _require_gpu(a, weight, w_scale, c, bias)
    if silu_mul and defer_reduce:
        raise SlmError("silu_mul and defer_reduce cannot be combined")
    if fp8 and weight.dtype not in (torch.float8_e4m3fn, torch.uint8):
        raise SlmError(f"fp8_linear takes float8_e4m3fn weights (or their bytes), not {weight.dtype}")
    if a.dim() != 2 or c.dim() != 2 or weight.dim() != 2 or a.stride(1) != 1 or c.stride(1) != 1 or \
            weight.stride(1) != 1:
        raise SlmError("A [M, K], W [N, K] and C [M, N] must be 2-D with contiguous rows")
    N, K = weight.shape
    if a.size(1) != K or c.size(1) != (N // 2 if silu_mul else N) or a.size(0) != c.size(0):
        raise SlmError(f"{name} shape mismatch")
    if (not fp8 and a.dtype != weight.dtype) or c.dtype != a.dtype or (bias is not None and bias.dtype != a.dtype):
        raise SlmError("activation / bias / output dtypes must match" if fp8 else
                       "activation / weight / bias / output dtypes must match")
    if bias is not None and (bias.dim() != 1 or bias.numel() != N or not bias.is_contiguous()):
        raise SlmError("bias must be a contiguous [N] tensor")
    if w_scale is not None and (w_scale.dtype != torch.float32 or w_scale.dim() != 1 or w_scale.numel() != N or
                                not w_scale.is_contiguous()):
        raise SlmError("w_scale must be a contiguous fp32 [N] tensor (expand a per-tensor scale on the host)")
    g = _lib.Fp8LinearArgs() if fp8 else _lib.LinearArgs()
    g.a, g.w, g.c = a.data_ptr(), weight.data_ptr(), c.data_ptr()
    g.bias = bias.data_ptr() if bias is not None else None
    if fp8:
        g.w_scale = w_scale.data_ptr() if w_scale is not None else None
    g.M, g.K, g.N = a.size(0), K, N
    g.lda, g.ldw, g.ldc = a.stride(0), weight.stride(0), c.stride(0)
    g.dtype = _dtype_code(a)
    g.flags = _lib.SLM_LINEAR_SHARES_CHIP if _chip_flag() else 0
    if silu_mul:
        g.flags |= _lib.SLM_LINEAR_SILU_MUL
    if defer_reduce:
        g.flags |= _lib.SLM_LINEAR_DEFER_REDUCE
    g.workspace, g.workspace_bytes = None, 0
    return g


def _linear_plan(entry: str, g) -> "_lib.LinearPlanInfo":
    info = _lib.LinearPlanInfo()
    check(getattr(_lib.lib(), entry + "_plan")(C.byref(g), C.byref(info)), entry + "_plan")
    return info


def linear_plan(a: torch.Tensor, weight: torch.Tensor, c: torch.Tensor, bias: Optional[torch.Tensor] = None,
                defer_reduce: bool = False, silu_mul: bool = False) -> "_lib.LinearPlanInfo":
    """The launch linear() would give these very arguments now, under the tuning knobs in force
    (slm_linear_plan): row tiles, waves, grid, K slices.  A host-side query: nothing runs on the GPU."""
    return _linear_plan("slm_linear", _linear_args(a, weight, None, c, bias, defer_reduce, silu_mul))


def _run_linear(entry: str, g, dev: torch.device, defer_reduce: bool) -> DeferredPartials:
    """Workspace, launch and deferred-slab handle of slm_linear / slm_fp8_linear / slm_mxfp4_linear (`entry`) over the
    argument block g"""
    L = _lib.lib()
    if g.M == 0:
        return DeferredPartials()
    deferred = getattr(L, entry + "_deferred_splits")(C.byref(g)) if defer_reduce else 0
    # (section 20 declares no _workspace_bytes query: the plan carries the size)
    need = _linear_plan(entry, g).workspace_bytes if entry == "slm_mxfp4_linear" else \
        getattr(L, entry + "_workspace_bytes")(C.byref(g))
    ws = None
    if need:
        # deferred slabs live in their own buffer (gptq_gemm: nothing else's scratch may overwrite them)
        ws = _grow(_deferred_ws, need, dev, "deferred split-K buffer") if deferred \
            else reserve_workspace(need, dev)
        g.workspace, g.workspace_bytes = ws.data_ptr(), ws.numel()
    check(getattr(L, entry)(C.byref(g), _stream()), entry)
    if deferred:
        key = _dev_key(dev)
        gen = _deferred_gen.get((key, 0), 0) + 1
        _deferred_gen[(key, 0)] = gen  # any older handle on this buffer is now stale
        return DeferredPartials(g.workspace, deferred, g.M * g.N, key, gen, ws, 0)
    return DeferredPartials()


def linear(a: torch.Tensor, weight: torch.Tensor, c: torch.Tensor, bias: Optional[torch.Tensor] = None,
           defer_reduce: bool = False, silu_mul: bool = False) -> DeferredPartials:
    """F::linear on unquantised weights (parallel_linear.cpp): C[M, N] = A[M, K] . W[N, K]^T (+ bias), fp32
    accumulate, one rounding, written into the pre-allocated `c`.  `weight` is the checkpoint tensor
    [N, K] (rows contiguous, any row stride): it is streamed as it is, never repacked.

    defer_reduce / the returned handle: as gptq_gemm -- a call that is split over K leaves its fp32 slabs
    in the deferred buffer for rms_norm / apply_rotary_pos_emb / gemma_sandwich_norm(partials=handle) and
    does NOT write `c` (truthy handle); otherwise `c` is written and the handle is falsy.

    silu_mul: rows [0, N/2) of `weight` are the gate, [N/2, N) the up projection and `c` is [M, N/2] =
    silu(gate) * up -- the bits of linear() followed by silu_and_mul()."""
    return _run_linear("slm_linear", _linear_args(a, weight, None, c, bias, defer_reduce, silu_mul), a.device,
                       defer_reduce)


# ---------------------------------------------------------------------------------------
# fp8 (e4m3) weight-only linear: slm_hip.h section 15
# ---------------------------------------------------------------------------------------
FP8_E4M3_MAX = 448.0


def quantize_fp8_weight(w: torch.Tensor, per: str = "channel"):
    """Load-time quantisation of a weight [N, K] to OCP e4m3fn (torch ops; nothing on the hot path):
    (w8 [N, K] float8_e4m3fn, scale fp32 [N]) with scale = amax / 448 per output channel ("channel") or of the
    whole tensor, repeated ("tensor"); an all-zero row (tensor) gets scale 1.  w ~ w8.float() * scale[:, None]."""
    if per not in ("channel", "tensor"):
        raise ValueError(f"per must be 'channel' or 'tensor', not {per!r}")
    if w.dim() != 2:
        raise ValueError("quantize_fp8_weight takes a 2-D weight [N, K]")
    wf = w.float()
    amax = wf.abs().amax(dim=1) if per == "channel" else wf.abs().amax().expand(w.size(0))
    scale = torch.where(amax > 0, amax / FP8_E4M3_MAX, torch.ones_like(amax)).contiguous()
    w8 = (wf / scale[:, None]).clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX).to(torch.float8_e4m3fn)
    return w8, scale


def fp8_linear_plan(a: torch.Tensor, w8: torch.Tensor, w_scale: Optional[torch.Tensor], c: torch.Tensor,
                    bias: Optional[torch.Tensor] = None, defer_reduce: bool = False,
                    silu_mul: bool = False) -> "_lib.LinearPlanInfo":
    """The launch fp8_linear() would give these very arguments now (slm_fp8_linear_plan); a host-side query."""
    return _linear_plan("slm_fp8_linear", _linear_args(a, w8, w_scale, c, bias, defer_reduce, silu_mul, fp8=True))


def fp8_linear(a: torch.Tensor, w8: torch.Tensor, w_scale: Optional[torch.Tensor], c: torch.Tensor,
               bias: Optional[torch.Tensor] = None, defer_reduce: bool = False,
               silu_mul: bool = False) -> DeferredPartials:
    """W8A16 linear (marlin::fp8_gemm's job over the checkpoint tensor): C[M, N] = T((A[M, K] . e4m3(W8[N, K])^T) *
    w_scale[N] + bias), fp32 accumulate, the scale applied to the fp32 sum, one rounding.  `w8` is the checkpoint's
    float8_e4m3fn weight [N, K] (rows contiguous, row stride a multiple of 16), streamed as bytes and converted in
    registers; `w_scale` fp32 [N] or None (1.0).  defer_reduce, silu_mul and the returned handle: as linear()."""
    return _run_linear("slm_fp8_linear", _linear_args(a, w8, w_scale, c, bias, defer_reduce, silu_mul, fp8=True),
                       a.device, defer_reduce)


# ---------------------------------------------------------------------------------------
# MXFP4 (e2m1 + e8m0 block scale) weight-only linear: slm_hip.h section 20
# ---------------------------------------------------------------------------------------
MXFP4_BLOCK = 32
# e2m1: 1 sign, 2 exponent (bias 1), 1 mantissa bit; codes 0..7, bit 3 is the sign
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def mxfp4_bytes(t: torch.Tensor, what: str = "weight") -> torch.Tensor:
    """The uint8 view of an MXFP4 checkpoint tensor: uint8 as it is, a weight also as torch.float4_e2m1fn_x2 or in the
    [N, K/32, 16] form of gpt-oss `*_blocks` (flattened to [N, K/2]), a scale (`what` ends in "scale") also as
    torch.float8_e8m0fnu.  Anything else -- the other tensor's typed dtype included: swapped keys -- is a TypeError."""
    typed = "float8_e8m0fnu" if what.endswith("scale") else "float4_e2m1fn_x2"
    if t.dtype != torch.uint8 and t.dtype != getattr(torch, typed, None):
        raise TypeError(f"mxfp4 linear: {what} must be uint8 bytes (or {typed}), not "
                        f"{t.dtype} (quantize_mxfp4_weight makes them; nothing is quantised on load)")
    if t.dtype != torch.uint8:
        t = t.view(torch.uint8)
    if t.dim() == 3:
        if t.size(2) != MXFP4_BLOCK // 2:
            raise ValueError(f"{what}: the blocked form is [N, K/32, 16], not {tuple(t.shape)}")
        t = t.reshape(t.size(0), -1)
    return t


def quantize_mxfp4_weight(w: torch.Tensor):
    """Load-time quantisation of a weight [N, K] (K % 32 == 0) to OCP MXFP4 (torch ops; nothing on the hot path):
    (packed uint8 [N, K/2], scale uint8 [N, K/32]).  Per block of 32 consecutive k the shared exponent is
    floor(log2(amax)) - 2 (2 = e2m1's largest exponent), stored as the e8m0 byte e = exponent + 127 clamped to
    [1, 254]; an all-zero block gets e = 127.  Elements are w / 2^(e - 127) rounded to nearest even onto the e2m1 grid
    {0, .5, 1, 1.5, 2, 3, 4, 6} and saturated at 6.  A byte's low nibble is the lower k.
    w ~ dequantize_mxfp4_weight(packed, scale, dtype)."""
    if w.dim() != 2 or w.size(1) % MXFP4_BLOCK:
        raise ValueError("quantize_mxfp4_weight takes a 2-D weight [N, K] with K % 32 == 0")
    N, K = w.shape
    blocks = w.float().reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = blocks.abs().amax(dim=2)
    _, ex = torch.frexp(amax)                                # amax = m 2^ex, m in [0.5, 1): floor(log2) = ex - 1
    e = torch.where(amax > 0, (ex - 1 - 2 + 127).clamp(1, 254), torch.full_like(ex, 127)).to(torch.int32)
    x = torch.ldexp(blocks, (127 - e)[:, :, None]).abs()     # exact: a power of two
    # round to nearest even per region of the grid: steps 0.5 below 2, 1 below 4, 2 above; saturate at 6
    q = torch.where(x < 2, torch.round(x * 2) / 2, torch.where(x < 4, torch.round(x), torch.round(x / 2) * 2)).clamp(max=6)
    idx = torch.where(q < 2, q * 2, torch.where(q < 4, q + 2, q / 2 + 4)).to(torch.int32)
    codes = (idx | (((blocks < 0) & (q > 0)).to(torch.int32) << 3)).reshape(N, K)
    packed = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8).contiguous()
    return packed, e.to(torch.uint8).contiguous()


def dequantize_mxfp4_weight(packed: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.float32):
    """[N, K] of `dtype` = e2m1(code) * 2^(e - 127), the low nibble of a byte first; exact wherever the product is a
    normal number of `dtype` (bf16: e in [2, 252]; f16: e in [114, 140]).  e = 255 (the MX NaN) gives NaN."""
    packed, scale = mxfp4_bytes(packed), mxfp4_bytes(scale, "weight_scale")
    N, K = packed.size(0), 2 * packed.size(1)
    if scale.dim() != 2 or tuple(scale.shape) != (N, K // MXFP4_BLOCK) or K % MXFP4_BLOCK:
        raise ValueError(f"weight_scale must be [N, K/32] = {(N, K // MXFP4_BLOCK)}, not {tuple(scale.shape)}")
    codes = torch.stack((packed & 0xF, packed >> 4), dim=2).reshape(N, K).long()
    table = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float64, device=packed.device)
    e = scale.to(torch.int32).repeat_interleave(MXFP4_BLOCK, dim=1)
    val = torch.ldexp(table[codes], e - 127)
    return torch.where(e == 255, torch.full_like(val, float("nan")), val).to(dtype)


def _mxfp4_args(a, w, w_scale, c, bias, defer_reduce: bool, silu_mul: bool):
    """Checks and argument block of mxfp4_linear() and its plan query: slm_linear_args over nibble bytes, plus the
    block scales and their row stride"""
    _require_gpu(a, w, w_scale, c, bias)
    if silu_mul and defer_reduce:
        raise SlmError("silu_mul and defer_reduce cannot be combined")
    if w_scale is None:
        raise SlmError("mxfp4_linear needs the e8m0 block scales [N, K/32]")
    try:
        w, w_scale = mxfp4_bytes(w), mxfp4_bytes(w_scale, "w_scale")
    except (TypeError, ValueError) as e:
        raise SlmError(str(e)) from None
    if a.dim() != 2 or c.dim() != 2 or w.dim() != 2 or w_scale.dim() != 2 or a.stride(1) != 1 or c.stride(1) != 1 or \
            w.stride(1) != 1 or w_scale.stride(1) != 1:
        raise SlmError("A [M, K], W [N, K/2], w_scale [N, K/32] and C [M, N] must be 2-D with contiguous rows")
    N, K = w.size(0), 2 * w.size(1)
    if a.size(1) != K or c.size(1) != (N // 2 if silu_mul else N) or a.size(0) != c.size(0) or K % MXFP4_BLOCK or \
            tuple(w_scale.shape) != (N, K // MXFP4_BLOCK):
        raise SlmError("mxfp4_linear shape mismatch")
    if c.dtype != a.dtype or (bias is not None and bias.dtype != a.dtype):
        raise SlmError("activation / bias / output dtypes must match")
    if bias is not None and (bias.dim() != 1 or bias.numel() != N or not bias.is_contiguous()):
        raise SlmError("bias must be a contiguous [N] tensor")
    g = _lib.Mxfp4LinearArgs()
    g.a, g.w, g.c = a.data_ptr(), w.data_ptr(), c.data_ptr()
    g.bias = bias.data_ptr() if bias is not None else None
    g.w_scale, g.lds = w_scale.data_ptr(), w_scale.stride(0)
    g.M, g.K, g.N = a.size(0), K, N
    g.lda, g.ldw, g.ldc = a.stride(0), w.stride(0), c.stride(0)
    g.dtype = _dtype_code(a)
    g.flags = _lib.SLM_LINEAR_SHARES_CHIP if _chip_flag() else 0
    if silu_mul:
        g.flags |= _lib.SLM_LINEAR_SILU_MUL
    if defer_reduce:
        g.flags |= _lib.SLM_LINEAR_DEFER_REDUCE
    g.workspace, g.workspace_bytes = None, 0
    return g


def mxfp4_linear_plan(a: torch.Tensor, w: torch.Tensor, w_scale: torch.Tensor, c: torch.Tensor,
                      bias: Optional[torch.Tensor] = None, defer_reduce: bool = False,
                      silu_mul: bool = False) -> "_lib.LinearPlanInfo":
    """The launch mxfp4_linear() would give these very arguments now (slm_mxfp4_linear_plan); a host-side query."""
    return _linear_plan("slm_mxfp4_linear", _mxfp4_args(a, w, w_scale, c, bias, defer_reduce, silu_mul))


def mxfp4_linear(a: torch.Tensor, w: torch.Tensor, w_scale: torch.Tensor, c: torch.Tensor,
                 bias: Optional[torch.Tensor] = None, silu_mul: bool = False,
                 defer_reduce: bool = False) -> DeferredPartials:
    """W4A16 linear over an OCP MXFP4 checkpoint: C[M, N] = T(A[M, K] . T(e2m1(W[N, K]) * 2^(e[N, K/32] - 127))^T +
    bias), fp32 accumulate, one rounding.  `w` is the checkpoint's packed weight, uint8 [N, K/2] (low nibble = lower
    k; rows contiguous, row stride a multiple of 16), `w_scale` its e8m0 bytes uint8 [N, K/32] (any row stride); both
    are streamed as they are and converted in registers.  defer_reduce, silu_mul and the returned handle: as
    linear()."""
    return _run_linear("slm_mxfp4_linear", _mxfp4_args(a, w, w_scale, c, bias, defer_reduce, silu_mul), a.device,
                       defer_reduce)


# ---------------------------------------------------------------------------------------
# glue ops (next rows f1/f2)
# ---------------------------------------------------------------------------------------
def rms_norm(out: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, eps: float,
             residual: Optional[torch.Tensor] = None,
             partials: Optional[DeferredPartials] = None) -> None:
    """kernel::rms_norm / rms_norm_residual (layernorm_kernels.cu:15,125).

    partials (truthy): `x` was NOT written -- the gptq_gemm(..., defer_reduce=True) that returned
    this handle left fp32 split-K slabs [splits, tokens, dim] in the deferred buffer; the norm sums
    them itself (same order and rounding as the reduce kernel: identical bits, one launch less).
    A handle is valid until the next deferred GEMM on the same device (checked)."""
    L = _lib.lib()
    _require_gpu(out, x, weight, residual)
    if not (x.is_contiguous() and out.is_contiguous() and weight.is_contiguous()):
        raise SlmError("rms_norm needs contiguous tensors")
    if residual is not None and not residual.is_contiguous():
        raise SlmError("rms_norm needs a contiguous residual")
    dim = x.size(-1)
    res_ptr = residual.data_ptr() if residual is not None else None
    if partials:
        if not isinstance(partials, DeferredPartials):
            raise SlmError("rms_norm(partials=...) takes the handle gptq_gemm(defer_reduce=True) returned")
        partials.check(x.device, x.numel(), "rms_norm(partials=...)")
        check(L.slm_rms_norm_splitk(out.data_ptr(), partials.ptr, partials.splits, weight.data_ptr(),
                                    res_ptr, x.numel() // dim, dim, float(eps), _dtype_code(x),
                                    _stream()), "slm_rms_norm_splitk")
        return
    check(L.slm_rms_norm(out.data_ptr(), x.data_ptr(), weight.data_ptr(), res_ptr,
                         x.numel() // dim, dim, float(eps), _dtype_code(x), _stream()),
          "slm_rms_norm")


def layer_norm(out: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
               eps: float) -> None:
    """kernel::layer_norm (layernorm_kernels.cu:231-256): out = T((x - mean) * rsqrt(var + eps) * weight
    + bias) per row, fp32 statistics; bias None = no bias (bias.defined() false in the reference)."""
    L = _lib.lib()
    _require_gpu(out, x, weight, bias)
    if not (x.is_contiguous() and out.is_contiguous() and weight.is_contiguous()) or \
            (bias is not None and not bias.is_contiguous()):
        raise SlmError("layer_norm needs contiguous tensors")
    dim = x.size(-1)
    if weight.numel() != dim or (bias is not None and bias.numel() != dim) or out.shape != x.shape:
        raise SlmError("layer_norm: weight / bias / out do not match the input's last dimension")
    check(L.slm_layer_norm(out.data_ptr(), x.data_ptr(), weight.data_ptr(),
                           bias.data_ptr() if bias is not None else None, x.numel() // dim, dim, float(eps),
                           _dtype_code(x), _stream()), "slm_layer_norm")


GELU_NEW, GELU_FAST = 0, 1


def _gelu(x: torch.Tensor, kind: int, with_mul: bool, out: Optional[torch.Tensor]) -> torch.Tensor:
    L = _lib.lib()
    _require_gpu(x, out)
    if x.dim() != 2 or not x.is_contiguous():
        raise SlmError("gelu needs a contiguous [n_tokens, d] input")
    d = x.size(1) // 2 if with_mul else x.size(1)
    if with_mul and x.size(1) % 2:
        raise SlmError("gelu_with_mul needs an even number of columns")
    if out is None:
        out = torch.empty(x.size(0), d, dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (x.size(0), d) or not out.is_contiguous() or out.dtype != x.dtype:
        raise SlmError("gelu: out must be a contiguous [n_tokens, d] tensor of the input's dtype")
    check(L.slm_gelu(out.data_ptr(), x.data_ptr(), x.size(0), d, kind, 1 if with_mul else 0, _dtype_code(x),
                     _stream()), "slm_gelu")
    return out


def gelu_new(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """kernel::gelu_new (activation_kernels.cu:111-114): 0.5 x (1 + tanh(0.79788456 (x + 0.044715 x^3)))."""
    return _gelu(x, GELU_NEW, False, out)


def gelu_fast(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """kernel::gelu_fast (activation_kernels.cu:116-119): 0.5 x (1 + tanh(0.79788456 x (1 + 0.044715 x^2)))."""
    return _gelu(x, GELU_FAST, False, out)


def gelu_new_with_mul(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """kernel::gelu_new_with_mul (activation_kernels.cu:128-135): gelu_new(x[:, :d]) * x[:, d:]."""
    return _gelu(x, GELU_NEW, True, out)


def gelu_fast_with_mul(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """kernel::gelu_fast_with_mul (activation_kernels.cu:137-144)."""
    return _gelu(x, GELU_FAST, True, out)


# ---------------------------------------------------------------------------------------
# Gemma family (slm_hip.h section 12)
# ---------------------------------------------------------------------------------------
def _gemma_norm(what: str, dim: int, n_tokens: int, dtype_of: torch.Tensor, eps: float, **ptrs) -> None:
    g = _lib.GemmaNormArgs()
    for name, t in ptrs.items():
        if isinstance(t, torch.Tensor):
            if not t.is_contiguous():
                raise SlmError(f"{what} needs contiguous tensors ({name})")
            setattr(g, name, t.data_ptr())
        elif t is not None:
            setattr(g, name, t)
    g.n_tokens, g.dim, g.dtype, g.eps = n_tokens, dim, _dtype_code(dtype_of), float(eps)
    check(_lib.lib().slm_gemma_norm(C.byref(g), _stream()), "slm_gemma_norm")


def _same_t(what: str, ref: torch.Tensor, **tensors) -> None:
    for name, t in tensors.items():
        if t is not None and t.dtype != ref.dtype:
            raise SlmError(f"{what}: {name} is {t.dtype}, expected {ref.dtype}")


def gemma_rms_norm(out: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, eps: float) -> None:
    """kernel::gemma_rms_norm (layernorm_kernels.cu:66-117): out = T(x * rsqrt(mean(x^2) + eps) * (1 + weight)),
    fp32 arithmetic and one rounding.  out may be x."""
    _require_gpu(out, x, weight)
    dim = x.size(-1)
    if weight.numel() != dim or out.shape != x.shape:
        raise SlmError("gemma_rms_norm: weight / out do not match the input")
    _same_t("gemma_rms_norm", x, out=out, weight=weight)
    _gemma_norm("gemma_rms_norm", dim, x.numel() // dim, x, eps, out=out, x=x, pre_weight=weight)


def gemma_sandwich_norm(out: Optional[torch.Tensor], x: torch.Tensor, post_weight: Optional[torch.Tensor],
                        residual: torch.Tensor, pre_weight: Optional[torch.Tensor], eps: float,
                        partials: Optional[DeferredPartials] = None) -> None:
    """The Gemma-2 sandwich (gemma2.h:186-204) in one launch: y = GN(x, post_weight) (None: y = x),
    residual = T(y + residual) in place, out = GN(residual, pre_weight) (pre_weight and out both None: skipped).

    partials (truthy): `x` was NOT written -- it only gives the shape; the gptq_gemm(..., defer_reduce=True)
    that returned the handle left fp32 split-K slabs, which the kernel sums and rounds as rms_norm(partials=...)
    does (identical bits to the reduced x, one launch less)."""
    _require_gpu(out, x, post_weight, residual, pre_weight)
    dim = x.size(-1)
    if residual.shape != x.shape or (out is not None and out.shape != x.shape):
        raise SlmError("gemma_sandwich_norm: residual / out do not match the input")
    if (out is None) != (pre_weight is None):
        raise SlmError("gemma_sandwich_norm: out and pre_weight go together")
    for w in (post_weight, pre_weight):
        if w is not None and w.numel() != dim:
            raise SlmError("gemma_sandwich_norm: a weight does not match the input's last dimension")
    _same_t("gemma_sandwich_norm", x, out=out, post_weight=post_weight, residual=residual, pre_weight=pre_weight)
    kw = dict(out=out, post_weight=post_weight, residual=residual, pre_weight=pre_weight)
    if partials:
        if not isinstance(partials, DeferredPartials):
            raise SlmError("gemma_sandwich_norm(partials=...) takes the handle gptq_gemm(defer_reduce=True) returned")
        partials.check(x.device, x.numel(), "gemma_sandwich_norm(partials=...)")
        kw.update(partials=partials.ptr, n_splits=partials.splits)
    else:
        kw.update(x=x)
    _gemma_norm("gemma_sandwich_norm", dim, x.numel() // dim, x, eps, **kw)


def gemma_embed_norm(out: torch.Tensor, residual: torch.Tensor, table: torch.Tensor, token_ids: torch.Tensor,
                     x_scale: float, weight: torch.Tensor, eps: float) -> None:
    """Embedding, Gemma's scale and the first input norm (gemma2.h:236-238,270) in one launch:
    residual = T(table[token_ids] * x_scale), out = GN(residual, weight).  x_scale is rounded to the tensors'
    dtype first, as the reference's T(sqrt(hidden)) is, which makes the product exact before its rounding."""
    _require_gpu(out, residual, table, token_ids, weight)
    if table.dim() != 2 or token_ids.dtype != torch.int32 or token_ids.dim() != 1:
        raise SlmError("gemma_embed_norm takes a [vocab, dim] table and int32 [n_tokens] ids")
    dim, n = table.size(1), token_ids.numel()
    if tuple(out.shape) != (n, dim) or tuple(residual.shape) != (n, dim) or weight.numel() != dim:
        raise SlmError("gemma_embed_norm: out / residual / weight do not match [n_tokens, dim]")
    _same_t("gemma_embed_norm", table, out=out, residual=residual, weight=weight)
    scale = torch.tensor(float(x_scale), dtype=table.dtype).float().item()
    _gemma_norm("gemma_embed_norm", dim, n, table, eps, out=out, residual=residual, table=table,
                token_ids=token_ids, pre_weight=weight, vocab=table.size(0), x_scale=scale)


def soft_cap(x: torch.Tensor, cap: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = T(cap * tanh(x / cap)) (gemma2.h:341-342; one pass and ONE rounding where the reference's three
    element-wise ops round three times).  out defaults to x: in place."""
    _require_gpu(x, out)
    if out is None:
        out = x
    if x.dim() < 1 or not x.is_contiguous() or not out.is_contiguous() or out.shape != x.shape or \
            out.dtype != x.dtype:
        raise SlmError("soft_cap needs contiguous x / out of one shape and dtype")
    row = x.size(-1)
    check(_lib.lib().slm_soft_cap(out.data_ptr(), x.data_ptr(), x.numel() // max(row, 1), row, float(cap),
                                  _dtype_code(x), _stream()), "slm_soft_cap")
    return out


def apply_rotary_pos_emb(query: torch.Tensor, key: torch.Tensor, positions: torch.Tensor,
                         cos_sin: torch.Tensor, rotary_dim: int, interleaved: bool,
                         value: Optional[torch.Tensor] = None,
                         slot_ids: Optional[torch.Tensor] = None,
                         key_cache: Optional[torch.Tensor] = None,
                         value_cache: Optional[torch.Tensor] = None,
                         partials: Optional["DeferredPartials"] = None) -> None:
    """kernel::apply_rotary_pos_emb (pos_embedding_kernels.cu:83-121), in place on query/key
    [n_tokens, n_heads, head_dim]; with value/slot_ids/caches given it also performs the KV
    append that follows it in AttentionImpl::forward (attention.cpp:36-42) in the same launch.

    partials (truthy): query / key / value are the three column slices of ONE fused-qkv GEMM
    output that was NOT written -- gptq_gemm(..., defer_reduce=True) left fp32 split-K slabs
    behind; the kernel sums them itself (same order and rounding as the reduce kernel: identical
    bits, one launch less) and WRITES query (rotated), key (rotated) and value."""
    L = _lib.lib()
    _require_gpu(query, key, positions, cos_sin, value, slot_ids, key_cache, value_cache)
    if query.stride(-1) != 1 or key.stride(-1) != 1 or query.stride(1) != query.size(2) or \
            key.stride(1) != key.size(2):
        raise SlmError("query/key must be contiguous in their last two dims")
    if positions.dtype != torch.int32 or not cos_sin.is_contiguous():
        raise SlmError("positions must be int32; cos_sin contiguous")
    is_f32 = 1 if cos_sin.dtype == torch.float32 else 0
    if not is_f32 and cos_sin.dtype != query.dtype:
        raise SlmError("cos_sin must be fp32 or the activation dtype")
    if not positions.is_contiguous() or positions.numel() != query.size(0):
        raise SlmError("positions must be contiguous int32 [n_tokens]")
    if key.size(0) != query.size(0) or key.size(2) != query.size(2) or key.dtype != query.dtype:
        raise SlmError("query / key token counts, head_dim and dtype must match")
    append = slot_ids is not None
    if append:
        # same contract as set_kv_cache: the kernel scatters dense [n_kv_heads, head_dim] rows
        # through int32 slot ids
        if value is None or key_cache is None or value_cache is None:
            raise SlmError("append needs value, key_cache and value_cache")
        if slot_ids.dtype != torch.int32 or not slot_ids.is_contiguous() or \
                slot_ids.numel() != query.size(0):
            raise SlmError("slot_ids must be contiguous int32 [n_tokens]")
        if value.dim() != 3 or value.shape != key.shape or value.dtype != key.dtype or \
                value.stride(-1) != 1 or value.stride(-2) != value.size(-1):
            raise SlmError("value must be [n_tokens, n_kv_heads, head_dim], contiguous in its last "
                           "two dims, same dtype as key")
        for t in (key_cache, value_cache):
            if not t.is_contiguous() or t.dtype != key.dtype or t.dim() != 3 or \
                    tuple(t.shape[1:]) != tuple(key.shape[1:]):
                raise SlmError("caches must be contiguous [n_slots, n_kv_heads, head_dim] of the "
                               "activation dtype")
    if partials:
        if not isinstance(partials, DeferredPartials):
            raise SlmError("apply_rotary_pos_emb(partials=...) takes the handle gptq_gemm(defer_reduce=True) returned")
        n_cols = (query.size(1) + 2 * key.size(1)) * query.size(2)
        partials.check(query.device, query.size(0) * n_cols, "apply_rotary_pos_emb(partials=...)")
        if value is None or value.shape != key.shape or value.stride(-1) != 1 or \
                value.stride(-2) != value.size(-1):
            raise SlmError("partials: value must be the [n_tokens, n_kv_heads, head_dim] slice of the qkv buffer")
        # the three slices must be [q | k | v] of one row-major [n_tokens, n_cols] buffer
        es = query.element_size()
        one_row = query.size(0) == 1  # (the stride of a size-1 dimension is arbitrary)
        if not ((one_row or query.stride(0) == key.stride(0) == value.stride(0) == n_cols) and
                key.data_ptr() == query.data_ptr() + query.size(1) * query.size(2) * es and
                value.data_ptr() == key.data_ptr() + key.size(1) * key.size(2) * es):
            raise SlmError("partials: query / key / value must be the [q | k | v] column slices of "
                           "the fused qkv GEMM output")
        ts = n_cols  # token stride of all three slices
        check(L.slm_rope_kv_append_splitk(
            partials.ptr, partials.splits, query.data_ptr(), ts, key.data_ptr(),
            ts, value.data_ptr(), ts, positions.data_ptr(),
            cos_sin.data_ptr(), is_f32, int(rotary_dim), 1 if interleaved else 0,
            slot_ids.data_ptr() if append else None, key_cache.data_ptr() if append else None,
            value_cache.data_ptr() if append else None, query.size(0), query.size(1), key.size(1),
            query.size(2), _dtype_code(query), _stream()), "slm_rope_kv_append_splitk")
        return
    check(L.slm_rope_kv_append(
        query.data_ptr(), query.stride(0), key.data_ptr(), key.stride(0),
        value.data_ptr() if append else None, value.stride(0) if append else 0,
        positions.data_ptr(), cos_sin.data_ptr(), is_f32, int(rotary_dim),
        1 if interleaved else 0, slot_ids.data_ptr() if append else None,
        key_cache.data_ptr() if append else None, value_cache.data_ptr() if append else None,
        query.size(0), query.size(1), key.size(1), query.size(2), _dtype_code(query), _stream()),
        "slm_rope_kv_append")


def qk_norm_rope_kv_append(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, q_norm_weight: torch.Tensor,
                           k_norm_weight: torch.Tensor, eps: float, positions: torch.Tensor, cos_sin: torch.Tensor,
                           interleaved: bool, slot_ids: Optional[torch.Tensor] = None,
                           key_cache: Optional[torch.Tensor] = None, value_cache: Optional[torch.Tensor] = None,
                           partials: Optional[DeferredPartials] = None) -> None:
    """The QK-norm prologue in one launch (slm_hip.h section 19): every head of query [T, H, D] and key [T, KV, D]
    RMS-normalised over its D values with q_norm_weight / k_norm_weight [D] (rms_norm's bits), then rotated by
    cos_sin[positions] over the whole head (apply_rotary_pos_emb's bits), in place; with slot_ids the rotated key
    and value also go to their cache slot (a negative id appends nothing).  The tensors may be column slices of one
    fused qkv GEMM output.

    partials (truthy): the fused [q | k | v] GEMM output was NOT written -- linear / fp8_linear / gptq_gemm(...,
    defer_reduce=True) left fp32 split-K slabs behind; the kernel sums them itself (the reduce kernel's order and
    rounding: identical bits, one launch less) and WRITES query, key and value."""
    L = _lib.lib()
    _require_gpu(query, key, value, q_norm_weight, k_norm_weight, positions, cos_sin, slot_ids, key_cache, value_cache)
    for t in (query, key, value):
        if t.dim() != 3 or t.stride(2) != 1 or t.stride(1) != t.size(2) or t.dtype != query.dtype:
            raise SlmError("query / key / value must be [n_tokens, heads, head_dim] of one dtype, contiguous in "
                           "their last two dims")
    T, D = query.size(0), query.size(2)
    if key.size(0) != T or key.size(2) != D or value.shape != key.shape:
        raise SlmError("query / key / value token counts and head_dim must match; value like key")
    if positions.dtype != torch.int32 or not positions.is_contiguous() or positions.numel() != T:
        raise SlmError("positions must be contiguous int32 [n_tokens]")
    for w in (q_norm_weight, k_norm_weight):
        if w.dtype != query.dtype or not w.is_contiguous() or w.numel() != D:
            raise SlmError("q_norm_weight / k_norm_weight must be contiguous [head_dim] of the activation dtype")
    is_f32 = 1 if cos_sin.dtype == torch.float32 else 0
    if (not is_f32 and cos_sin.dtype != query.dtype) or not cos_sin.is_contiguous():
        raise SlmError("cos_sin must be contiguous, fp32 or the activation dtype")
    append = slot_ids is not None
    if append:
        if key_cache is None or value_cache is None:
            raise SlmError("append needs key_cache and value_cache")
        if slot_ids.dtype != torch.int32 or not slot_ids.is_contiguous() or slot_ids.numel() != T:
            raise SlmError("slot_ids must be contiguous int32 [n_tokens]")
        for t in (key_cache, value_cache):
            if not t.is_contiguous() or t.dtype != key.dtype or t.dim() != 3 or \
                    tuple(t.shape[1:]) != tuple(key.shape[1:]):
                raise SlmError("caches must be contiguous [n_slots, n_kv_heads, head_dim] of the activation dtype")
    tail = (q_norm_weight.data_ptr(), k_norm_weight.data_ptr(), float(eps), positions.data_ptr(),
            cos_sin.data_ptr(), is_f32, cos_sin.size(-1), 1 if interleaved else 0,
            slot_ids.data_ptr() if append else None, key_cache.data_ptr() if append else None,
            value_cache.data_ptr() if append else None, T, query.size(1), key.size(1), D, _dtype_code(query),
            _stream())
    if partials:
        if not isinstance(partials, DeferredPartials):
            raise SlmError("qk_norm_rope_kv_append(partials=...) takes the handle a deferred GEMM returned")
        partials.check(query.device, T * (query.size(1) + 2 * key.size(1)) * D, "qk_norm_rope_kv_append(partials=...)")
        check(L.slm_qk_norm_rope_kv_append_splitk(partials.ptr, partials.splits, query.data_ptr(), query.stride(0),
                                                  key.data_ptr(), key.stride(0), value.data_ptr(), value.stride(0),
                                                  *tail), "slm_qk_norm_rope_kv_append_splitk")
        return
    check(L.slm_qk_norm_rope_kv_append(query.data_ptr(), query.stride(0), key.data_ptr(), key.stride(0),
                                       value.data_ptr(), value.stride(0), *tail), "slm_qk_norm_rope_kv_append")


def silu_and_mul(out: torch.Tensor, x: torch.Tensor) -> None:
    """kernel::act_and_mul with SiLU (activation_kernels.cu:84): out = silu(x[:, :d]) * x[:, d:]."""
    L = _lib.lib()
    _require_gpu(out, x)
    if not (x.is_contiguous() and out.is_contiguous()):
        raise SlmError("silu_and_mul needs contiguous tensors")
    d = x.size(-1) // 2
    check(L.slm_silu_mul(out.data_ptr(), x.data_ptr(), x.numel() // (2 * d), d, _dtype_code(x),
                         _stream()), "slm_silu_mul")


# ---------------------------------------------------------------------------------------
# logits processing and sampling (include/slm_hip.h section 8, csrc/sampling.hip)
#   apply_temperature_penalty / apply_repetition_penalty / apply_frequency_presence_penalty
#       <- llm::kernel::*  src/kernels/sampling/sampling_kernels.h:7-25 (in place, rounded once)
#   sample / logits_process
#       <- LogitsProcessor::create + Sampler::forward, src/engine/worker.cpp:154-187 (fused)
# ---------------------------------------------------------------------------------------


def _logits_dtype_code(t: torch.Tensor) -> int:
    return _lib.SLM_F32 if t.dtype == torch.float32 else _dtype_code(t)


def _rows(t: Optional[torch.Tensor], n: int, dtype: torch.dtype, what: str) -> Optional[torch.Tensor]:
    """A per-row parameter as a contiguous [n] tensor of `dtype` (the reference keeps them as
    [n, 1] columns in the logits dtype: parameters.h:42-67, logits_processor.h:126-127)."""
    if t is None:
        return None
    _require_gpu(t)
    t = t.reshape(-1)
    if t.numel() != n:
        raise SlmError(f"{what}: {t.numel()} values for {n} rows")
    return t if (t.dtype == dtype and t.is_contiguous()) else t.to(dtype).contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _sampling_call(fn, what: str, logits: torch.Tensor, *, frequency_penalties=None, presence_penalties=None,
                   repetition_penalties=None, temperatures=None, top_k=None, top_p=None, unique_token_ids=None,
                   unique_token_counts=None, unique_token_lens=None, do_sample=None, seeds=None, positions=None,
                   next_tokens=None, processed=None, probs=None, logprobs=None, top_logprobs=None,
                   top_tokens=None) -> None:
    _require_gpu(logits)
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise SlmError("logits must be [n_rows, vocab] with contiguous rows")
    n, V = logits.shape
    a = _lib.SamplingArgs()
    a.logits, a.logits_stride, a.dtype = logits.data_ptr(), logits.stride(0), _logits_dtype_code(logits)
    a.n_rows, a.vocab = n, V
    keep = []  # converted copies stay alive until the launch is issued

    def rows(t, dtype, name):
        t = _rows(t, n, dtype, name)
        keep.append(t)
        return _ptr(t)
    a.frequency_penalties = rows(frequency_penalties, torch.float32, "frequency_penalties")
    a.presence_penalties = rows(presence_penalties, torch.float32, "presence_penalties")
    a.repetition_penalties = rows(repetition_penalties, torch.float32, "repetition_penalties")
    a.temperatures = rows(temperatures, torch.float32, "temperatures")
    a.top_p = rows(top_p, torch.float32, "top_p")
    a.top_k = rows(top_k, torch.int64, "top_k")
    a.do_sample = rows(do_sample, torch.bool, "do_sample")
    a.seeds = rows(seeds, torch.int64, "seeds")   # uint64 seeds travel as their int64 bit pattern
    a.positions = rows(positions, torch.int32, "positions")
    if unique_token_ids is not None:
        _require_gpu(unique_token_ids)
        ids = unique_token_ids.reshape(n, -1)
        ids = ids if (ids.dtype == torch.int64 and ids.is_contiguous()) else ids.to(torch.int64).contiguous()
        a.unique_ids, a.max_unique = ids.data_ptr(), ids.size(1)
        keep.append(ids)
        if unique_token_counts is not None:
            cnt = unique_token_counts.reshape(n, -1)
            if cnt.size(1) != ids.size(1):
                raise SlmError("unique_token_counts and unique_token_ids differ in shape")
            cnt = cnt if (cnt.dtype == torch.int32 and cnt.is_contiguous()) else cnt.to(torch.int32).contiguous()
            a.unique_counts = cnt.data_ptr()
            keep.append(cnt)
        a.unique_lens = rows(unique_token_lens, torch.int32, "unique_token_lens")
    for t, name in ((next_tokens, "next_tokens"), (logprobs, "logprobs")):
        if t is not None and (not t.is_contiguous() or t.numel() != n):
            raise SlmError(f"{name} must be contiguous with one entry per row")
    if next_tokens is not None and next_tokens.dtype != torch.int32:
        raise SlmError("next_tokens must be int32")
    a.next_tokens, a.logprobs = _ptr(next_tokens), _ptr(logprobs)
    if processed is not None:
        if processed.dtype != logits.dtype or processed.shape != logits.shape or processed.stride(1) != 1:
            raise SlmError("processed must have the logits' dtype and shape")
        a.processed, a.processed_stride = processed.data_ptr(), processed.stride(0)
    if probs is not None:
        if probs.dtype != torch.float32 or not probs.is_contiguous() or probs.shape != logits.shape:
            raise SlmError("probs must be contiguous fp32 [n_rows, vocab]")
        a.probs = probs.data_ptr()
    if top_logprobs is not None or top_tokens is not None:
        if top_logprobs is None or top_tokens is None or not top_logprobs.is_contiguous() or \
                not top_tokens.is_contiguous() or top_tokens.dtype != torch.int32 or \
                top_logprobs.dtype != torch.float32 or top_logprobs.shape != top_tokens.shape:
            raise SlmError("top_logprobs (fp32) and top_tokens (int32) must be contiguous [n_rows, n_top]")
        a.top_logprobs, a.top_tokens, a.n_top = top_logprobs.data_ptr(), top_tokens.data_ptr(), top_tokens.size(-1)
    L = _lib.lib()
    need = L.slm_sample_workspace_bytes(C.byref(a))
    if need:
        ws = _grow(_sampling_ws, need, logits.device, "sampling workspace")
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    check(fn(C.byref(a), _stream()), what)


def sample(logits: torch.Tensor, next_tokens: Optional[torch.Tensor] = None, **kw) -> torch.Tensor:
    """Steps 1-7 of slm_hip.h section 8 in one launch: penalties, temperature, top-k / top-p, greedy or
    seeded random sampling per row, optional processed logits / probs / logprobs / top logprobs (pass
    the output tensors).  Returns next_tokens (int32 [n_rows])."""
    if next_tokens is None:
        next_tokens = torch.empty(logits.size(0), dtype=torch.int32, device=logits.device)
    _sampling_call(_lib.lib().slm_sample, "slm_sample", logits, next_tokens=next_tokens, **kw)
    return next_tokens


def logits_process(logits: torch.Tensor, processed: Optional[torch.Tensor] = None, **kw) -> torch.Tensor:
    """Steps 1-5 only (penalties, temperature, top-k / top-p) into `processed` (default: in place),
    rounded once to the logits dtype; filtered tokens are -inf."""
    processed = logits if processed is None else processed
    _sampling_call(_lib.lib().slm_logits_process, "slm_logits_process", logits, processed=processed, **kw)
    return processed


def apply_temperature_penalty(logits: torch.Tensor, temperatures: torch.Tensor) -> None:
    """llm::kernel::apply_temperature_penalty (penalty_kernels.cu:9-55): logits *= 1 / t in place."""
    logits_process(logits, temperatures=temperatures)


def apply_repetition_penalty(logits: torch.Tensor, token_ids: torch.Tensor, token_ids_lens: torch.Tensor,
                             penalities: torch.Tensor) -> None:
    """llm::kernel::apply_repetition_penalty (penalty_kernels.cu:57-111), in place."""
    logits_process(logits, unique_token_ids=token_ids, unique_token_lens=token_ids_lens,
                   repetition_penalties=penalities)


def apply_frequency_presence_penalty(logits: torch.Tensor, token_ids: torch.Tensor, token_counts: torch.Tensor,
                                     token_ids_lens: torch.Tensor, frequency_penalties: torch.Tensor,
                                     presence_penalties: torch.Tensor) -> None:
    """llm::kernel::apply_frequency_presence_penalty (penalty_kernels.cu:113-182), in place."""
    logits_process(logits, unique_token_ids=token_ids, unique_token_counts=token_counts,
                   unique_token_lens=token_ids_lens, frequency_penalties=frequency_penalties,
                   presence_penalties=presence_penalties)


# ---------------------------------------------------------------------------------------
#   rejection_sample
#       <- RejectionSampler::forward / random_sample / greedy_sample,
#          src/speculative/rejection_sampler.cpp:22-226 (two launches, no host sync)
# ---------------------------------------------------------------------------------------
def _rows3(t: torch.Tensor, n: int, rows: int, V: int, what: str):
    """A [n, >= rows, V] tensor with contiguous vocab: its sequence and row strides (elements)."""
    if t.dim() != 3 or t.size(0) != n or t.size(1) < rows or t.size(2) != V or t.stride(2) != 1:
        raise SlmError(f"{what} must be [n_seqs, {rows}, vocab] with contiguous rows, got {tuple(t.shape)}")
    return t.stride(0), t.stride(1)


def rejection_sample_workspace_bytes(n_seqs: int, k: int) -> int:
    a = _lib.RejectionArgs()
    a.n_seqs, a.k = n_seqs, k
    return int(_lib.lib().slm_rejection_sample_workspace_bytes(C.byref(a)))


def rejection_sample(draft_token_ids: torch.Tensor, draft_probs: Optional[torch.Tensor], target: torch.Tensor,
                     bonus_token_ids: torch.Tensor, *, target_is_probs: bool = False, mask_out_rejected: bool = False,
                     do_sample=None, seeds=None, positions=None, uniform=None, next_tokens=None,
                     accepted_lens=None, logprobs=None, top_logprobs=None, top_tokens=None) -> torch.Tensor:
    """slm_hip.h section 9 in two launches: validates k draft tokens per sequence against the target rows.
    draft_token_ids [n, k]; draft_probs [n, k, V] fp32 (slm_sample's probs; None = every sequence greedy);
    target [n, k + 1, V] logits (f16 / bf16 / fp32) or, with target_is_probs, [n, k, V] fp32 probabilities;
    bonus_token_ids [n].  Strided draft / target rows are read in place.  Returns next_tokens
    (int32 [n, k + 1]); pass accepted_lens ([n] int32), logprobs ([n, k + 1]) and top_logprobs /
    top_tokens ([n, k + 1, n_top]) to have them written."""
    _require_gpu(draft_token_ids, draft_probs, target, bonus_token_ids)
    if draft_token_ids.dim() != 2:
        raise SlmError("draft_token_ids must be [n_seqs, k]")
    n, k = draft_token_ids.shape
    if target.dim() != 3:
        raise SlmError("target must be [n_seqs, rows, vocab]")
    V = target.size(2)
    a = _lib.RejectionArgs()
    a.n_seqs, a.k, a.vocab = n, k, V
    a.target_is_probs, a.mask_out_rejected = int(bool(target_is_probs)), int(bool(mask_out_rejected))
    if target_is_probs and target.dtype != torch.float32:
        raise SlmError("a probability target must be fp32")
    a.dtype = _logits_dtype_code(target)
    a.target = target.data_ptr()
    a.target_seq_stride, a.target_row_stride = _rows3(target, n, k if target_is_probs else k + 1, V, "target")
    keep = []

    def rows(t, dtype, name, count=n):
        if t is None:
            return None
        _require_gpu(t)
        t = t.reshape(-1)
        if t.numel() != count:
            raise SlmError(f"{name}: {t.numel()} values, expected {count}")
        t = t if (t.dtype == dtype and t.is_contiguous()) else t.to(dtype).contiguous()
        keep.append(t)
        return t.data_ptr()
    a.draft_token_ids = rows(draft_token_ids, torch.int32, "draft_token_ids", n * k)
    a.bonus_token_ids = rows(bonus_token_ids, torch.int32, "bonus_token_ids")
    if draft_probs is not None:
        if draft_probs.dtype != torch.float32:
            raise SlmError("draft_probs must be fp32")
        a.draft_probs = draft_probs.data_ptr()
        a.draft_seq_stride, a.draft_row_stride = _rows3(draft_probs, n, k, V, "draft_probs")
    a.do_sample = rows(do_sample, torch.bool, "do_sample")
    a.seeds = rows(seeds, torch.int64, "seeds")  # uint64 seeds travel as their int64 bit pattern
    a.positions = rows(positions, torch.int32, "positions")
    a.uniform = rows(uniform, torch.float32, "uniform", n * k)
    if next_tokens is None:
        next_tokens = torch.empty(n, k + 1, dtype=torch.int32, device=target.device)
    for t, name, cnt, dt in ((next_tokens, "next_tokens", n * (k + 1), torch.int32),
                             (accepted_lens, "accepted_lens", n, torch.int32),
                             (logprobs, "logprobs", n * (k + 1), torch.float32)):
        if t is not None and (not t.is_contiguous() or t.numel() != cnt or t.dtype != dt):
            raise SlmError(f"{name} must be contiguous {dt} with {cnt} entries")
    a.next_tokens, a.accepted_lens, a.logprobs = _ptr(next_tokens), _ptr(accepted_lens), _ptr(logprobs)
    if top_logprobs is not None or top_tokens is not None:
        if top_logprobs is None or top_tokens is None or not top_logprobs.is_contiguous() or \
                not top_tokens.is_contiguous() or top_tokens.dtype != torch.int32 or \
                top_logprobs.dtype != torch.float32 or top_logprobs.shape != top_tokens.shape or \
                top_tokens.numel() != n * (k + 1) * top_tokens.size(-1):
            raise SlmError("top_logprobs (fp32) and top_tokens (int32) must be contiguous [n_seqs, k + 1, n_top]")
        a.top_logprobs, a.top_tokens, a.n_top = top_logprobs.data_ptr(), top_tokens.data_ptr(), top_tokens.size(-1)
    L = _lib.lib()
    need = L.slm_rejection_sample_workspace_bytes(C.byref(a))
    if need:
        ws = _grow(_rejection_ws, need, target.device, "rejection workspace")
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    check(L.slm_rejection_sample(C.byref(a), _stream()), "slm_rejection_sample")
    return next_tokens


# ---------------------------------------------------------------------------------------
# mixture of experts (include/slm_hip.h section 10): routing, block alignment, grouped int4 GEMM
#   moe_topk_softmax / moe_grouped_topk_sigmoid <- llm::kernel::topk_softmax / grouped_topk_sigmoid
#   moe_align_block / moe_sum                   <- llm::kernel::moe::permute_align_block / sum_out
#   moe_w4_grouped_gemm                         <- the grouped GEMM of src/kernels/gemm/ over int4 experts
#   moe_grouped_gemm                            <- the grouped GEMM of src/kernels/gemm/ itself (dense f16 / bf16)
#   moe_fp8_grouped_gemm                        <- the same over fp8 (e4m3) experts with channel scales (section 16)
# ---------------------------------------------------------------------------------------
MOE_GEMM_BLOCK = _lib.SLM_MOE_GEMM_BLOCK


class PackedMoeW4:
    """The packed int4 weights of E experts of one shape, stacked: wq [E, K * N / 8] and sz [E, G * N] int32,
    expert e in row e (each row is one PackedW4 image, include/slm_hip.h section 3)."""

    def __init__(self, wq, sz, K, N, group_size, dtype, fmt, paired=False):
        self.wq, self.sz = wq, sz
        self.K, self.N, self.group_size, self.dtype = K, N, group_size, dtype
        self.fmt, self.paired = fmt, paired
        self.n_experts = wq.size(0)

    def expert(self, e: int) -> PackedW4:
        """Expert e as a dense-GEMM weight (a view: no copy)."""
        return PackedW4(self.wq[e], self.sz[e], None, self.K, self.N, self.group_size, self.dtype, self.paired)

    def nbytes(self) -> int:
        return (self.wq.numel() + self.sz.numel()) * 4


def moe_stack_experts(experts, fmt: int) -> PackedMoeW4:
    """Stack per-expert PackedW4 images (all of one shape, no act-order perm) into a PackedMoeW4.
    fmt: _lib.SLM_W4_GPTQ or _lib.SLM_W4_AWQ, the checkpoint format they were packed from."""
    p0 = experts[0]
    for p in experts:
        if p.perm is not None:
            raise SlmError("act-order (perm) and 8-bit experts are not supported by the grouped GEMM")
        if (p.K, p.N, p.group_size, p.dtype, p.paired) != (p0.K, p0.N, p0.group_size, p0.dtype, p0.paired):
            raise SlmError("all experts must share K, N, group_size, dtype and pairing")
    wq = torch.stack([p.wq.view(-1) for p in experts]).contiguous()
    sz = torch.stack([p.sz.view(-1) for p in experts]).contiguous()
    return PackedMoeW4(wq, sz, p0.K, p0.N, p0.group_size, p0.dtype, fmt, p0.paired)


def _route_out(logits, topk, weights, indices):
    _require_gpu(logits, weights, indices)
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise SlmError("router logits must be contiguous fp32 [n_tokens, n_experts]")
    T = logits.size(0)
    if weights is None:
        weights = torch.empty(T, topk, dtype=torch.float32, device=logits.device)
    if indices is None:
        indices = torch.empty(T, topk, dtype=torch.int32, device=logits.device)
    for t, dt, name in ((weights, torch.float32, "topk_weights"), (indices, torch.int32, "topk_indices")):
        if t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != (T, topk):
            raise SlmError(f"{name} must be contiguous {dt} [n_tokens, topk]")
    return weights, indices


def moe_topk_softmax(logits: torch.Tensor, topk: int, renormalize: bool = False,
                     weights: Optional[torch.Tensor] = None, indices: Optional[torch.Tensor] = None):
    """llm::kernel::topk_softmax: the k largest logits per token (ties: the lower expert id), weights =
    softmax over all experts at those; renormalize: divided by their sum.  Returns (weights, indices)."""
    weights, indices = _route_out(logits, topk, weights, indices)
    check(_lib.lib().slm_moe_topk_softmax(logits.data_ptr(), weights.data_ptr(), indices.data_ptr(), logits.size(0),
                                          logits.size(1), topk, 1 if renormalize else 0, _stream()),
          "slm_moe_topk_softmax")
    return weights, indices


def moe_grouped_topk_sigmoid(logits: torch.Tensor, correction_bias: torch.Tensor, n_expert_groups: int,
                             topk_group: int, topk: int, scaling_factor: float,
                             weights: Optional[torch.Tensor] = None, indices: Optional[torch.Tensor] = None):
    """llm::kernel::grouped_topk_sigmoid (DeepSeek-V3 style routing).  Returns (weights, indices)."""
    weights, indices = _route_out(logits, topk, weights, indices)
    _require_gpu(correction_bias)
    if correction_bias.dtype != torch.float32 or not correction_bias.is_contiguous() or \
            correction_bias.numel() != logits.size(1):
        raise SlmError("correction_bias must be contiguous fp32 [n_experts]")
    check(_lib.lib().slm_moe_grouped_topk_sigmoid(logits.data_ptr(), correction_bias.data_ptr(), weights.data_ptr(),
                                                  indices.data_ptr(), logits.size(0), logits.size(1),
                                                  n_expert_groups, topk_group, topk, float(scaling_factor),
                                                  _stream()), "slm_moe_grouped_topk_sigmoid")
    return weights, indices


def moe_router_splits(n_experts: int, hidden: int, dtype: torch.dtype) -> int:
    """The K slices slm_moe_router spreads a row tile over: a function of (E, hidden, dtype), never of T."""
    s = C.c_int32(0)
    code = SLM_BF16 if dtype == torch.bfloat16 else SLM_F16 if dtype == torch.float16 else _lib.SLM_F32
    check(_lib.lib().slm_moe_router_splits(n_experts, hidden, code, C.byref(s)), "slm_moe_router_splits")
    return s.value


def moe_router(x: torch.Tensor, gate_weight: torch.Tensor, topk: int, *, scoring: str = "softmax",
               renormalize: bool = True, correction_bias: Optional[torch.Tensor] = None, n_expert_groups: int = 1,
               topk_group: int = 1, scaling_factor: float = 1.0, weights: Optional[torch.Tensor] = None,
               indices: Optional[torch.Tensor] = None, logits_out: Optional[torch.Tensor] = None):
    """The fused router (slm_hip.h section 17): logits = x [T, hidden] . gate_weight [E, hidden]^T in fp32 and the
    routing of moe_topk_softmax (scoring = "softmax") or moe_grouped_topk_sigmoid ("grouped_sigmoid") on them, in
    one launch.  x and gate_weight are f16 / bf16 with contiguous rows (row strides may be padded; gate_weight is
    the checkpoint tensor, no transpose, no fp32 copy).  logits_out: optional contiguous fp32 [T, E] that receives
    the logits.  A token's result depends on that token alone.  Returns (weights, indices)."""
    _require_gpu(x, gate_weight, correction_bias, weights, indices, logits_out)
    if scoring not in ("softmax", "grouped_sigmoid"):
        raise SlmError(f"unknown scoring {scoring}")
    if x.dim() != 2 or gate_weight.dim() != 2 or x.stride(1) != 1 or gate_weight.stride(1) != 1 or \
            x.size(1) != gate_weight.size(1):
        raise SlmError("moe_router: x [T, hidden] and gate_weight [E, hidden] with contiguous rows")
    if x.dtype != gate_weight.dtype:
        raise SlmError("moe_router: x and gate_weight must share one dtype")
    T, H = x.shape
    E = gate_weight.size(0)
    if weights is None:
        weights = torch.empty(T, topk, dtype=torch.float32, device=x.device)
    if indices is None:
        indices = torch.empty(T, topk, dtype=torch.int32, device=x.device)
    for t, dt, shape, name in ((weights, torch.float32, (T, topk), "weights"),
                               (indices, torch.int32, (T, topk), "indices"),
                               (logits_out, torch.float32, (T, E), "logits_out")):
        if t is not None and (t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != shape):
            raise SlmError(f"moe_router: {name} must be contiguous {dt} {list(shape)}")
    if correction_bias is not None and (correction_bias.dtype != torch.float32 or
                                        not correction_bias.is_contiguous() or correction_bias.numel() != E):
        raise SlmError("correction_bias must be contiguous fp32 [n_experts]")
    if scoring == "grouped_sigmoid" and correction_bias is None:
        raise SlmError("moe_router: grouped_sigmoid needs correction_bias")
    a = _lib.MoeRouterArgs()
    a.x, a.gate_w = x.data_ptr(), gate_weight.data_ptr()
    a.correction_bias = correction_bias.data_ptr() if correction_bias is not None else None
    a.weights, a.indices = weights.data_ptr(), indices.data_ptr()
    a.logits_out = logits_out.data_ptr() if logits_out is not None else None
    a.n_tokens, a.hidden = T, H
    a.ldx = x.stride(0) if T > 1 else max(x.stride(0), H)
    a.ldw = gate_weight.stride(0) if E > 1 else max(gate_weight.stride(0), H)
    a.n_experts, a.topk, a.dtype = E, topk, _dtype_code(x)
    a.scoring = _lib.SLM_ROUTER_SOFTMAX if scoring == "softmax" else _lib.SLM_ROUTER_GROUPED_SIGMOID
    a.renormalize = 1 if renormalize else 0
    a.n_expert_groups, a.topk_group, a.scaling_factor = n_expert_groups, topk_group, float(scaling_factor)
    need = C.c_size_t(0)
    check(_lib.lib().slm_moe_router_workspace_bytes(T, E, H, a.dtype, C.byref(need)), "slm_moe_router_workspace_bytes")
    if need.value:
        ws = reserve_workspace(need.value, x.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    check(_lib.lib().slm_moe_router(C.byref(a), _stream()), "slm_moe_router")
    return weights, indices


def moe_align_capacity(n_flat: int, n_experts: int, block_size: int):
    """(max_padded, max_blocks): the worst case of moe_align_block's outputs for n_flat = T * k assignments."""
    mp, mb = C.c_int64(0), C.c_int64(0)
    check(_lib.lib().slm_moe_align_capacity(n_flat, n_experts, block_size, C.byref(mp), C.byref(mb)),
          "slm_moe_align_capacity")
    return mp.value, mb.value


def moe_align_block(topk_ids: torch.Tensor, n_experts: int, block_size: int, sorted_token_idxes: torch.Tensor,
                    expert_ids: torch.Tensor, n_padded_tokens: torch.Tensor,
                    cu_sum: Optional[torch.Tensor] = None) -> None:
    """llm::kernel::moe::permute_align_block, with the flat indices of an expert in ascending order and the
    padding entries written by the kernel (include/slm_hip.h section 10)."""
    _require_gpu(topk_ids, sorted_token_idxes, expert_ids, n_padded_tokens, cu_sum)
    for t in (topk_ids, sorted_token_idxes, expert_ids, n_padded_tokens, cu_sum):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise SlmError("moe_align_block takes contiguous int32 tensors")
    if cu_sum is not None and cu_sum.numel() < n_experts + 1:
        raise SlmError("cu_sum needs n_experts + 1 entries")
    a = _lib.MoeAlignArgs()
    a.topk_ids, a.sorted_token_idxes = topk_ids.data_ptr(), sorted_token_idxes.data_ptr()
    a.expert_ids, a.n_padded_tokens = expert_ids.data_ptr(), n_padded_tokens.data_ptr()
    a.cu_sum = cu_sum.data_ptr() if cu_sum is not None else None
    a.n_flat = topk_ids.numel()
    a.sorted_capacity, a.blocks_capacity = sorted_token_idxes.numel(), expert_ids.numel()
    a.n_experts, a.block_size = n_experts, block_size
    check(_lib.lib().slm_moe_align_block(C.byref(a), _stream()), "slm_moe_align_block")


def moe_sum(inp: torch.Tensor, out: torch.Tensor) -> None:
    """llm::kernel::moe::sum_out: out [T, dim] = sum over j of inp [T, k, dim], fp32, one rounding."""
    _require_gpu(inp, out)
    if inp.dim() != 3 or not inp.is_contiguous() or not out.is_contiguous() or inp.dtype != out.dtype or \
            tuple(out.shape) != (inp.size(0), inp.size(2)):
        raise SlmError("moe_sum: input [T, k, dim] and output [T, dim] must be contiguous and of one dtype")
    check(_lib.lib().slm_moe_sum(out.data_ptr(), inp.data_ptr(), inp.size(0), inp.size(1), inp.size(2),
                                 _dtype_code(inp), _stream()), "slm_moe_sum")


def moe_sum_add(inp: torch.Tensor, addend: torch.Tensor, out: torch.Tensor) -> None:
    """out [T, dim] = sum over j of inp [T, k, dim], then + addend [T, dim] (the shared experts' output): fp32, that
    order, one rounding -- the bits of moe_sum over [T, k + 1, dim] with the addend as slot k (slm_moe_sum_add).
    `out` may be `addend`."""
    _require_gpu(inp, addend, out)
    if inp.dim() != 3 or not inp.is_contiguous() or not out.is_contiguous() or not addend.is_contiguous() or \
            inp.dtype != out.dtype or addend.dtype != out.dtype or \
            tuple(out.shape) != (inp.size(0), inp.size(2)) or addend.shape != out.shape:
        raise SlmError("moe_sum_add: input [T, k, dim], addend [T, dim] and output [T, dim] must be contiguous and "
                       "of one dtype")
    check(_lib.lib().slm_moe_sum_add(out.data_ptr(), inp.data_ptr(), addend.data_ptr(), inp.size(0), inp.size(1),
                                     inp.size(2), _dtype_code(inp), _stream()), "slm_moe_sum_add")


def moe_w4_grouped_gemm(a: torch.Tensor, experts: PackedMoeW4, c: torch.Tensor, sorted_token_idxes: torch.Tensor,
                        expert_ids: torch.Tensor, n_padded_tokens: torch.Tensor, a_div: int,
                        row_scale: Optional[torch.Tensor] = None, silu_mul: bool = False) -> None:
    """C[idx] = epilogue(A[idx // a_div] . dequant(W_e)) for the 32-row blocks moe_align_block(block_size = 32)
    produced.  a_div = topk when `a` holds one row per token, 1 when it holds one per (token, expert).
    silu_mul: paired (gate | up) experts, c is [n_flat, N / 2]; row_scale: fp32 [n_flat] routing weights applied
    to the fp32 accumulator.  The grid covers expert_ids.numel() blocks; the count in use is read on the device."""
    _require_gpu(a, c, sorted_token_idxes, expert_ids, n_padded_tokens, row_scale)
    if a.dim() != 2 or c.dim() != 2 or a.stride(1) != 1 or c.stride(1) != 1:
        raise SlmError("A and C must be 2-D with contiguous rows")
    if silu_mul and not experts.paired:
        raise SlmError("silu_mul=True needs experts packed with paired=True")
    n_flat = c.size(0)
    if a.size(1) != experts.K or c.size(1) != (experts.N // 2 if silu_mul else experts.N) or \
            a_div < 1 or a.size(0) * a_div < n_flat:
        raise SlmError("grouped GEMM shape mismatch")
    if a.dtype != experts.dtype or c.dtype != experts.dtype:
        raise SlmError("activation / output dtype must match the experts' scales dtype")
    for t in (sorted_token_idxes, expert_ids, n_padded_tokens):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise SlmError("sorted_token_idxes / expert_ids / n_padded_tokens must be contiguous int32")
    if sorted_token_idxes.numel() < expert_ids.numel() * MOE_GEMM_BLOCK:
        raise SlmError("sorted_token_idxes is shorter than expert_ids.numel() blocks of 32")
    if row_scale is not None and (row_scale.dtype != torch.float32 or not row_scale.is_contiguous() or
                                  row_scale.numel() != n_flat):
        raise SlmError("row_scale must be contiguous fp32 with one entry per row of C")
    g = _lib.MoeGemmArgs()
    g.a, g.wq, g.sz, g.c = a.data_ptr(), experts.wq.data_ptr(), experts.sz.data_ptr(), c.data_ptr()
    g.perm, g.bias = None, None
    g.row_scale = row_scale.data_ptr() if row_scale is not None else None
    g.sorted_token_idxes, g.expert_ids = sorted_token_idxes.data_ptr(), expert_ids.data_ptr()
    g.n_padded_tokens = n_padded_tokens.data_ptr()
    g.wq_expert_stride, g.sz_expert_stride = experts.wq.stride(0) * 4, experts.sz.stride(0) * 4
    g.n_flat, g.K, g.N = n_flat, experts.K, experts.N
    g.lda, g.ldc, g.group_size = a.stride(0), c.stride(0), experts.group_size
    g.a_div, g.n_experts, g.max_blocks = a_div, experts.n_experts, expert_ids.numel()
    g.dtype = _dtype_code(a)
    g.format = experts.fmt | (_lib.SLM_W4_PAIRED if experts.paired else 0)
    g.flags = _lib.SLM_W4_SILU_MUL if silu_mul else 0
    check(_lib.lib().slm_moe_w4a16_gemm(C.byref(g), _stream()), "slm_moe_w4a16_gemm")


def _moe_grouped_gemm(a, w, w_scale, c, sorted_token_idxes, expert_ids, n_padded_tokens, a_div, row_scale, silu_mul,
                      fp8: bool) -> None:
    """Checks, argument block and launch of moe_grouped_gemm(), or with fp8 of moe_fp8_grouped_gemm(): the same
    block plus w_scale, over e4m3 bytes (`w`) that do not share the activations' dtype"""
    _require_gpu(a, w, w_scale, c, sorted_token_idxes, expert_ids, n_padded_tokens, row_scale)
    if fp8 and w.dtype not in (torch.float8_e4m3fn, torch.uint8):
        raise SlmError(f"moe_fp8_grouped_gemm takes float8_e4m3fn weights (or their bytes), not {w.dtype}")
    if a.dim() != 2 or c.dim() != 2 or a.stride(1) != 1 or c.stride(1) != 1:
        raise SlmError("A and C must be 2-D with contiguous rows")
    if w.dim() != 3 or w.stride(2) != 1:
        raise SlmError("expert weights must be [n_experts, N, K] with k contiguous")
    E, N, K = w.shape
    n_flat = c.size(0)
    if a.size(1) != K or c.size(1) != (N // 2 if silu_mul else N) or a_div < 1 or a.size(0) * a_div < n_flat:
        raise SlmError("grouped GEMM shape mismatch")
    if fp8:
        if a.dtype not in (torch.float16, torch.bfloat16) or c.dtype != a.dtype:
            raise SlmError("activation and output must share one dtype, fp16 or bf16")
    elif a.dtype != w.dtype or c.dtype != w.dtype:
        raise SlmError("activation / output dtype must match the experts' dtype")
    if w_scale is not None and (w_scale.dtype != torch.float32 or tuple(w_scale.shape) != (E, N) or
                                w_scale.stride(1) != 1):
        raise SlmError("w_scale must be fp32 [n_experts, N] with contiguous rows (expand a per-tensor scale)")
    for t in (sorted_token_idxes, expert_ids, n_padded_tokens):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise SlmError("sorted_token_idxes / expert_ids / n_padded_tokens must be contiguous int32")
    if sorted_token_idxes.numel() < expert_ids.numel() * MOE_GEMM_BLOCK:
        raise SlmError("sorted_token_idxes is shorter than expert_ids.numel() blocks of 32")
    if row_scale is not None and (row_scale.dtype != torch.float32 or not row_scale.is_contiguous() or
                                  row_scale.numel() != n_flat):
        raise SlmError("row_scale must be contiguous fp32 with one entry per row of C")
    g = _lib.MoeFp8GemmArgs() if fp8 else _lib.MoeDenseGemmArgs()
    g.a, g.w, g.c = a.data_ptr(), w.data_ptr(), c.data_ptr()
    g.row_scale = row_scale.data_ptr() if row_scale is not None else None
    g.sorted_token_idxes, g.expert_ids = sorted_token_idxes.data_ptr(), expert_ids.data_ptr()
    g.n_padded_tokens = n_padded_tokens.data_ptr()
    # a single expert's stride(0) is not meaningful: what covers the expert will do (fp8: a multiple of 16)
    g.w_expert_stride = w.stride(0) if E > 1 else \
        max(w.stride(0), N * w.stride(1) if fp8 else (N - 1) * w.stride(1) + K)
    if fp8:
        g.w_scale = w_scale.data_ptr() if w_scale is not None else None
        g.w_scale_expert_stride = 0 if w_scale is None else \
            (w_scale.stride(0) if E > 1 else max(w_scale.stride(0), N))
    g.n_flat, g.K, g.N = n_flat, K, N
    g.lda, g.ldw, g.ldc = a.stride(0), w.stride(1), c.stride(0)
    g.a_div, g.n_experts, g.max_blocks = a_div, E, expert_ids.numel()
    g.dtype = _dtype_code(a)
    g.flags = _lib.SLM_MOE_SILU_MUL if silu_mul else 0
    entry = "slm_moe_fp8_gemm" if fp8 else "slm_moe_gemm"
    check(getattr(_lib.lib(), entry)(C.byref(g), _stream()), entry)


def moe_grouped_gemm(a: torch.Tensor, w: torch.Tensor, c: torch.Tensor, sorted_token_idxes: torch.Tensor,
                     expert_ids: torch.Tensor, n_padded_tokens: torch.Tensor, a_div: int,
                     row_scale: Optional[torch.Tensor] = None, silu_mul: bool = False) -> None:
    """C[idx] = epilogue(A[idx // a_div] . W[e]^T) over unquantised experts w [E, N, K] (the checkpoint layout,
    k contiguous; expert and row strides may be larger than dense), for the 32-row blocks
    moe_align_block(block_size = 32) produced.  silu_mul: rows [0, N/2) of an expert are the gate, [N/2, N) the up
    projection, c is [n_flat, N / 2]; row_scale: fp32 [n_flat] routing weights applied to the fp32 accumulator.
    The grid covers expert_ids.numel() blocks; the count in use is read on the device."""
    _moe_grouped_gemm(a, w, None, c, sorted_token_idxes, expert_ids, n_padded_tokens, a_div, row_scale, silu_mul,
                      fp8=False)


def moe_fp8_grouped_gemm(a: torch.Tensor, w8: torch.Tensor, w_scale: Optional[torch.Tensor], c: torch.Tensor,
                         sorted_token_idxes: torch.Tensor, expert_ids: torch.Tensor, n_padded_tokens: torch.Tensor,
                         a_div: int, row_scale: Optional[torch.Tensor] = None, silu_mul: bool = False) -> None:
    """moe_grouped_gemm over fp8 experts (slm_hip.h section 16): C[idx] = epilogue((A[idx // a_div] . e4m3(W8[e])^T)
    * w_scale[e]).  `w8` is [E, N, K] float8_e4m3fn (or its bytes as uint8), the checkpoint layout, k contiguous,
    expert and row strides may be padded (multiples of 16); `w_scale` fp32 [E, N] (rows contiguous, the expert
    stride may be padded) or None (1.0), applied to the fp32 accumulator before row_scale and the one rounding.
    silu_mul, row_scale, the aligned list and the grid: as moe_grouped_gemm."""
    _moe_grouped_gemm(a, w8, w_scale, c, sorted_token_idxes, expert_ids, n_padded_tokens, a_div, row_scale, silu_mul,
                      fp8=True)


def moe_mxfp4_grouped_gemm(a: torch.Tensor, w: torch.Tensor, w_scale: torch.Tensor, c: torch.Tensor,
                           sorted_token_idxes: torch.Tensor, expert_ids: torch.Tensor, n_padded_tokens: torch.Tensor,
                           a_div: int, row_scale: Optional[torch.Tensor] = None, silu_mul: bool = False) -> None:
    """moe_grouped_gemm over OCP MXFP4 experts (slm_hip.h section 21): C[idx] = epilogue(A[idx // a_div] .
    T(e2m1(W[e]) * 2^(w_scale[e] - 127))^T).  `w` is uint8 [E, N, K/2] (two e2m1 codes a byte, the low nibble the lower
    k; or torch.float4_e2m1fn_x2; or the [E, N, K/32, 16] blocks view of the same memory), the checkpoint layout, k
    contiguous, expert and row strides may be padded (multiples of 16); `w_scale` uint8 [E, N, K/32] e8m0 bytes (or
    torch.float8_e8m0fnu), rows contiguous, any row / expert stride and any base alignment.  Both are streamed as they
    are and converted in registers; the block scale goes through the converter, nothing touches the accumulator.
    silu_mul, row_scale, the aligned list and the grid: as moe_grouped_gemm."""
    _require_gpu(a, w, w_scale, c, sorted_token_idxes, expert_ids, n_padded_tokens, row_scale)
    if w_scale is None:
        raise SlmError("moe_mxfp4_grouped_gemm needs the e8m0 block scales [n_experts, N, K/32]")
    for t, typed, what in ((w, "float4_e2m1fn_x2", "w"), (w_scale, "float8_e8m0fnu", "w_scale")):
        if t.dtype != torch.uint8 and t.dtype != getattr(torch, typed, None):
            raise SlmError(f"moe_mxfp4_grouped_gemm: {what} must be uint8 bytes (or {typed}), not {t.dtype}")
    if w.dtype != torch.uint8:
        w = w.view(torch.uint8)
    if w_scale.dtype != torch.uint8:
        w_scale = w_scale.view(torch.uint8)
    if w.dim() == 4:  # [E, N, K/32, 16]: the same bytes as [E, N, K/2]
        if w.size(3) != MXFP4_BLOCK // 2 or w.stride(3) != 1 or w.stride(2) != MXFP4_BLOCK // 2:
            raise SlmError(f"the blocked form is [n_experts, N, K/32, 16] with contiguous rows, not {tuple(w.shape)}")
        w = w.as_strided((w.size(0), w.size(1), w.size(2) * w.size(3)), (w.stride(0), w.stride(1), 1),
                         w.storage_offset())
    if a.dim() != 2 or c.dim() != 2 or a.stride(1) != 1 or c.stride(1) != 1:
        raise SlmError("A and C must be 2-D with contiguous rows")
    if w.dim() != 3 or w.stride(2) != 1 or w_scale.dim() != 3 or w_scale.stride(2) != 1:
        raise SlmError("expert weights must be [n_experts, N, K/2] and scales [n_experts, N, K/32], k contiguous")
    E, N, K = w.size(0), w.size(1), 2 * w.size(2)
    n_flat = c.size(0)
    if K % MXFP4_BLOCK or tuple(w_scale.shape) != (E, N, K // MXFP4_BLOCK):
        raise SlmError(f"w_scale must be [n_experts, N, K/32] = {(E, N, K // MXFP4_BLOCK)}, not {tuple(w_scale.shape)}")
    if a.size(1) != K or c.size(1) != (N // 2 if silu_mul else N) or a_div < 1 or a.size(0) * a_div < n_flat:
        raise SlmError("grouped GEMM shape mismatch")
    if a.dtype not in (torch.float16, torch.bfloat16) or c.dtype != a.dtype:
        raise SlmError("activation and output must share one dtype, fp16 or bf16")
    for t in (sorted_token_idxes, expert_ids, n_padded_tokens):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise SlmError("sorted_token_idxes / expert_ids / n_padded_tokens must be contiguous int32")
    if sorted_token_idxes.numel() < expert_ids.numel() * MOE_GEMM_BLOCK:
        raise SlmError("sorted_token_idxes is shorter than expert_ids.numel() blocks of 32")
    if row_scale is not None and (row_scale.dtype != torch.float32 or not row_scale.is_contiguous() or
                                  row_scale.numel() != n_flat):
        raise SlmError("row_scale must be contiguous fp32 with one entry per row of C")
    g = _lib.MoeMxfp4GemmArgs()
    g.a, g.w, g.w_scale, g.c = a.data_ptr(), w.data_ptr(), w_scale.data_ptr(), c.data_ptr()
    g.row_scale = row_scale.data_ptr() if row_scale is not None else None
    g.sorted_token_idxes, g.expert_ids = sorted_token_idxes.data_ptr(), expert_ids.data_ptr()
    g.n_padded_tokens = n_padded_tokens.data_ptr()
    # a single expert's stride(0) is not meaningful: what covers the expert will do (the weights: a multiple of 16)
    g.w_expert_stride = w.stride(0) if E > 1 else max(w.stride(0), N * w.stride(1))
    g.w_scale_expert_stride = w_scale.stride(0) if E > 1 else max(w_scale.stride(0), N * w_scale.stride(1))
    g.n_flat, g.K, g.N = n_flat, K, N
    g.lda, g.ldw, g.ldc, g.lds = a.stride(0), w.stride(1), c.stride(0), w_scale.stride(1)
    g.a_div, g.n_experts, g.max_blocks = a_div, E, expert_ids.numel()
    g.dtype = _dtype_code(a)
    g.flags = _lib.SLM_MOE_SILU_MUL if silu_mul else 0
    check(_lib.lib().slm_moe_mxfp4_gemm(C.byref(g), _stream()), "slm_moe_mxfp4_gemm")


# ---------------------------------------------------------------------------------------
# MoE token permutation (slm_hip.h section 14; csrc/permute.hip)
#   permute_with_index_map / unpermute_with_index_map <- llm::kernel::moe::  (permutation_index_kernel.cu)
#   permute_with_mask_map / unpermute_with_mask_map   <- llm::kernel::moe::  (permutation_mask_kernel.cu)
# The four take and return what the reference's take and return; every buffer can be passed in (out= / row_id_map= /
# tokens_per_expert=) so that a caller allocates once and captures the calls in a graph.
# ---------------------------------------------------------------------------------------
PERMUTE_MAX_EXPERTS = 1024
_ROW_DTYPES = {torch.float16: SLM_F16, torch.bfloat16: SLM_BF16, torch.float32: _lib.SLM_F32}


def _row_dtype_code(t: torch.Tensor) -> int:
    if t.dtype not in _ROW_DTYPES:
        raise SlmError(f"token rows must be fp16, bf16 or fp32, got {t.dtype}")
    return _ROW_DTYPES[t.dtype]


def _i32_buffer(t: Optional[torch.Tensor], n: int, device, what: str) -> torch.Tensor:
    if t is None:
        return torch.empty(n, dtype=torch.int32, device=device)
    if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != n:
        raise SlmError(f"{what} must be contiguous int32 with {n} entries")
    return t


def permute_index_map(topk_ids: torch.Tensor, n_experts: int = PERMUTE_MAX_EXPERTS,
                      row_id_map: Optional[torch.Tensor] = None, tokens_per_expert: Optional[torch.Tensor] = None,
                      count: bool = False):
    """topk_ids [T, k] int32 -> row_id_map [k, T] int32: the permuted row of every (token, slot), expert-major and
    within an expert by ascending t * k + j; ids outside [0, n_experts) get -1.  count=True (or a tokens_per_expert
    buffer) also returns the rows per expert.  Returns (row_id_map, tokens_per_expert or None)."""
    _require_gpu(topk_ids, row_id_map, tokens_per_expert)
    if topk_ids.dim() != 2 or topk_ids.dtype != torch.int32 or not topk_ids.is_contiguous():
        raise SlmError("topk_ids must be contiguous int32 [n_tokens, topk]")
    T, k = topk_ids.shape
    row_id_map = _i32_buffer(row_id_map, k * T, topk_ids.device, "row_id_map").view(k, T)
    if count or tokens_per_expert is not None:
        tokens_per_expert = _i32_buffer(tokens_per_expert, n_experts, topk_ids.device, "tokens_per_expert")
    check(_lib.lib().slm_permute_index_map(topk_ids.data_ptr(), T, k, n_experts, row_id_map.data_ptr(),
                                           _ptr(tokens_per_expert), _stream()), "slm_permute_index_map")
    return row_id_map, tokens_per_expert


def permute_mask_map(routing_map: torch.Tensor, row_id_map: Optional[torch.Tensor] = None,
                     tokens_per_expert: Optional[torch.Tensor] = None, n_permuted: Optional[torch.Tensor] = None,
                     count: bool = False):
    """routing_map [T, E] bool (or uint8) -> row_id_map [E, T] int32: the permuted row of token t at expert e or -1,
    expert-major and within an expert by ascending token.  Returns (row_id_map, tokens_per_expert or None);
    n_permuted: an int32 [1] buffer that receives the number of mapped rows."""
    _require_gpu(routing_map, row_id_map, tokens_per_expert, n_permuted)
    if routing_map.dim() != 2 or routing_map.dtype not in (torch.bool, torch.uint8) or \
            not routing_map.is_contiguous():
        raise SlmError("routing_map must be contiguous bool [n_tokens, n_experts]")
    T, E = routing_map.shape
    row_id_map = _i32_buffer(row_id_map, E * T, routing_map.device, "row_id_map").view(E, T)
    if count or tokens_per_expert is not None:
        tokens_per_expert = _i32_buffer(tokens_per_expert, E, routing_map.device, "tokens_per_expert")
    if n_permuted is not None:
        n_permuted = _i32_buffer(n_permuted, 1, routing_map.device, "n_permuted")
    check(_lib.lib().slm_permute_mask_map(routing_map.data_ptr(), T, E, row_id_map.data_ptr(),
                                          _ptr(tokens_per_expert), _ptr(n_permuted), _stream()),
          "slm_permute_mask_map")
    return row_id_map, tokens_per_expert


def _rows_2d(t: torch.Tensor, what: str) -> None:
    if t.dim() != 2 or not t.is_contiguous():
        raise SlmError(f"{what} must be a contiguous [rows, dim] tensor")


def permute_rows(tokens: torch.Tensor, row_id_map: torch.Tensor, permuted: torch.Tensor) -> torch.Tensor:
    """permuted[row_id_map[m, t]] = tokens[t] for every mapped m; rows of `permuted` that no entry names keep what
    they held."""
    _require_gpu(tokens, row_id_map, permuted)
    _rows_2d(tokens, "tokens")
    _rows_2d(permuted, "permuted_tokens")
    T, dim = tokens.shape
    if permuted.dtype != tokens.dtype or permuted.size(1) != dim:
        raise SlmError("permuted_tokens must have the tokens' dtype and dim")
    if row_id_map.dtype != torch.int32 or not row_id_map.is_contiguous() or T == 0 and row_id_map.numel() or \
            T and row_id_map.numel() % T:
        raise SlmError("row_id_map must be contiguous int32 [n_maps, n_tokens]")
    n_maps = row_id_map.numel() // T if T else 1
    check(_lib.lib().slm_permute_rows(permuted.data_ptr(), tokens.data_ptr(), row_id_map.data_ptr(), T, n_maps, dim,
                                      permuted.size(0), _row_dtype_code(tokens), _stream()), "slm_permute_rows")
    return permuted


def unpermute_rows(permuted: torch.Tensor, row_id_map: torch.Tensor, probs: Optional[torch.Tensor], n_tokens: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[t] = sum over the mapped m of probs[t, m] * permuted[row_id_map[m, t]], fp32, one rounding; probs [T,
    n_maps] fp32 or of the tokens' dtype, None = 1."""
    _require_gpu(permuted, row_id_map, probs, out)
    _rows_2d(permuted, "permuted_tokens")
    dim = permuted.size(1)
    if out is None:
        out = torch.empty(n_tokens, dim, dtype=permuted.dtype, device=permuted.device)
    _rows_2d(out, "out")
    if out.dtype != permuted.dtype or tuple(out.shape) != (n_tokens, dim):
        raise SlmError("out must be [n_tokens, dim] of the permuted tokens' dtype")
    if row_id_map.dtype != torch.int32 or not row_id_map.is_contiguous() or \
            (n_tokens and row_id_map.numel() % n_tokens) or (not n_tokens and row_id_map.numel()):
        raise SlmError("row_id_map must be contiguous int32 [n_maps, n_tokens]")
    n_maps = row_id_map.numel() // n_tokens if n_tokens else 1
    pcode = _lib.SLM_F32
    if probs is not None:
        if probs.dtype not in (torch.float32, permuted.dtype) or not probs.is_contiguous() or \
                probs.numel() != n_tokens * n_maps:
            raise SlmError("probs must be contiguous [n_tokens, n_maps], fp32 or of the tokens' dtype")
        pcode = _row_dtype_code(probs)
    check(_lib.lib().slm_unpermute_rows(out.data_ptr(), permuted.data_ptr(), row_id_map.data_ptr(), _ptr(probs),
                                        pcode, n_tokens, n_maps, dim, permuted.size(0), _row_dtype_code(permuted),
                                        _stream()), "slm_unpermute_rows")
    return out


def _permuted_out(out: Optional[torch.Tensor], rows: int, tokens: torch.Tensor) -> torch.Tensor:
    if out is None:
        return torch.empty(rows, tokens.size(1), dtype=tokens.dtype, device=tokens.device)
    if out.dim() != 2 or out.size(0) < rows:
        raise SlmError(f"out needs at least {rows} rows")
    return out


def permute_with_index_map(tokens: torch.Tensor, indices: torch.Tensor, n_experts: int = PERMUTE_MAX_EXPERTS,
                           out: Optional[torch.Tensor] = None, row_id_map: Optional[torch.Tensor] = None,
                           tokens_per_expert: Optional[torch.Tensor] = None):
    """llm::kernel::moe::permute_with_index_map: tokens [T, dim], indices [T, k] int32 -> (permuted_tokens
    [T * k, dim] sorted by (expert, flat index), row_id_map [k, T]).  The reference is not told n_experts; the
    default is the kernels' upper bound and costs nothing but idle workgroups."""
    _require_gpu(tokens)
    _rows_2d(tokens, "tokens")
    row_id_map, _ = permute_index_map(indices, n_experts, row_id_map, tokens_per_expert)
    out = _permuted_out(out, indices.numel(), tokens)
    return permute_rows(tokens, row_id_map, out), row_id_map


def unpermute_with_index_map(permuted_tokens: torch.Tensor, row_id_map: torch.Tensor, probs: torch.Tensor,
                             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """llm::kernel::moe::unpermute_with_index_map: probs [T, k] -> tokens [T, dim]."""
    return unpermute_rows(permuted_tokens, row_id_map, probs, probs.size(0), out)


def permute_with_mask_map(tokens: torch.Tensor, routing_map: torch.Tensor, topk: int,
                          out: Optional[torch.Tensor] = None, row_id_map: Optional[torch.Tensor] = None,
                          tokens_per_expert: Optional[torch.Tensor] = None):
    """llm::kernel::moe::permute_with_mask_map: tokens [T, dim], routing_map [T, E] bool with topk experts per token
    -> (permuted_tokens [T * topk, dim] sorted by (expert, token), row_id_map [E, T])."""
    _require_gpu(tokens)
    _rows_2d(tokens, "tokens")
    row_id_map, _ = permute_mask_map(routing_map, row_id_map, tokens_per_expert)
    out = _permuted_out(out, tokens.size(0) * topk, tokens)
    return permute_rows(tokens, row_id_map, out), row_id_map


def unpermute_with_mask_map(permuted_tokens: torch.Tensor, row_id_map: torch.Tensor, probs: torch.Tensor,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """llm::kernel::moe::unpermute_with_mask_map: row_id_map [E, T], probs [T, E] -> tokens [T, dim]."""
    if row_id_map.dim() != 2:
        raise SlmError("row_id_map must be [n_experts, n_tokens]")
    return unpermute_rows(permuted_tokens, row_id_map, probs, row_id_map.size(1), out)


# ---------------------------------------------------------------------------------------
# multi-head latent attention (slm_hip.h section 11; csrc/mla.hip)
# ---------------------------------------------------------------------------------------
def _mla_args(out, q, q_rope, kv_cache, k_rope_cache, q_cu_lens, kv_cu_lens, block_table, block_cu_lens,
              block_size, max_q_len, max_kv_len, sm_scale, num_splits) -> "_lib.MlaArgs":
    _require_gpu(out, q, q_rope, kv_cache, k_rope_cache, q_cu_lens, kv_cu_lens, block_table, block_cu_lens)
    if out.dim() != 3 or q.dim() != 3 or q_rope.dim() != 3 or kv_cache.dim() != 2 or k_rope_cache.dim() != 2:
        raise SlmError("mla: out/q [n_tokens, n_heads, head_dim], q_rope [n_tokens, n_heads, rope_head_dim]; "
                       "caches [n_slots, head_dim] and [n_slots, rope_head_dim]")
    for t in (out, q, q_rope, kv_cache, k_rope_cache):
        if t.stride(-1) != 1:
            raise SlmError("mla: last dimension must be contiguous")
        if t.dtype != q.dtype:
            raise SlmError("mla: out/q/q_rope/kv_cache/k_rope_cache dtypes must match")
    for t in (q_cu_lens, kv_cu_lens, block_table, block_cu_lens):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise SlmError("index tensors must be contiguous int32")
    if out.shape != q.shape or q_rope.shape[:2] != q.shape[:2] or kv_cache.size(1) != q.size(2) or \
            k_rope_cache.size(1) != q_rope.size(2) or kv_cache.size(0) != k_rope_cache.size(0):
        raise SlmError("mla: shape mismatch between out / q / q_rope / caches")
    a = _lib.MlaArgs()
    a.out, a.q, a.q_rope = out.data_ptr(), q.data_ptr(), q_rope.data_ptr()
    a.kv_cache, a.k_rope_cache = kv_cache.data_ptr(), k_rope_cache.data_ptr()
    a.o_stride[0], a.o_stride[1] = out.stride(0), out.stride(1)
    a.q_stride[0], a.q_stride[1] = q.stride(0), q.stride(1)
    a.q_rope_stride[0], a.q_rope_stride[1] = q_rope.stride(0), q_rope.stride(1)
    a.kv_stride, a.k_rope_stride = kv_cache.stride(0), k_rope_cache.stride(0)
    a.q_cu_lens, a.kv_cu_lens = q_cu_lens.data_ptr(), kv_cu_lens.data_ptr()
    a.block_table, a.block_cu_lens = block_table.data_ptr(), block_cu_lens.data_ptr()
    a.dtype = _dtype_code(q)
    a.batch_size, a.n_tokens = q_cu_lens.numel() - 1, q.size(0)
    a.n_heads, a.head_dim, a.rope_head_dim = q.size(1), q.size(2), q_rope.size(2)
    a.block_size, a.max_q_len, a.max_kv_len = int(block_size), int(max_q_len), int(max_kv_len)
    a.sm_scale, a.num_splits = float(sm_scale), int(num_splits)
    a.workspace, a.workspace_bytes = None, 0
    return a


def mla_paged_kv(
    out: torch.Tensor,            # [n_tokens, n_heads, head_dim]
    q: torch.Tensor,              # [n_tokens, n_heads, head_dim]
    q_rope: torch.Tensor,         # [n_tokens, n_heads, rope_head_dim]
    kv_cache: torch.Tensor,       # [n_slots, head_dim]: the latent rows (K and V)
    k_rope_cache: torch.Tensor,   # [n_slots, rope_head_dim]
    q_cu_lens: torch.Tensor,      # [batch + 1] int32
    kv_cu_lens: torch.Tensor,     # [batch + 1] int32
    block_table: torch.Tensor,    # flattened first-slot ids, int32
    block_cu_lens: torch.Tensor,  # [batch + 1] int32
    block_size: int,
    max_q_len: int,
    max_kv_len: int,
    sm_scale: float,
    num_splits: int = 0,          # 0 = heuristic, > 0 forces the split-KV count
) -> None:
    """Multi-head latent attention over the paged latent cache (slm_mla_paged_kv; semantics of the reference's
    tests/mla_ref.h): writes `out` in place, async on the current stream."""
    L = _lib.lib()
    a = _mla_args(out, q, q_rope, kv_cache, k_rope_cache, q_cu_lens, kv_cu_lens, block_table, block_cu_lens,
                  block_size, max_q_len, max_kv_len, sm_scale, num_splits)
    if a.n_tokens == 0 or a.batch_size == 0:
        return
    need = L.slm_mla_paged_kv_workspace_bytes(C.byref(a))
    if need:
        ws = reserve_workspace(need, q.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    check(L.slm_mla_paged_kv(C.byref(a), _stream()), "slm_mla_paged_kv")


def mla_paged_kv_auto_splits(n_tokens: int, batch_size: int, n_heads: int, head_dim: int, max_q_len: int,
                             max_kv_len: int, dtype=torch.bfloat16) -> int:
    """Split-KV count the library's heuristic picks for these sizes (host-side only)."""
    a = _lib.MlaArgs()
    a.dtype = _lib.SLM_BF16 if dtype == torch.bfloat16 else _lib.SLM_F16
    a.batch_size, a.n_tokens, a.n_heads = int(batch_size), int(n_tokens), int(n_heads)
    a.head_dim, a.rope_head_dim = int(head_dim), 64
    a.max_q_len, a.max_kv_len = int(max_q_len), int(max_kv_len)
    return int(_lib.lib().slm_mla_paged_kv_auto_splits(C.byref(a)))


def mla_set_kv_cache(slot_ids: torch.Tensor, kv: torch.Tensor, k_rope: torch.Tensor, kv_cache: torch.Tensor,
                     k_rope_cache: torch.Tensor) -> None:
    """kv_cache[slot_ids[t]] = kv[t] and k_rope_cache[slot_ids[t]] = k_rope[t] in one launch (bit-exact; the
    sources may have any 16-byte aligned token stride)."""
    _require_gpu(slot_ids, kv, k_rope, kv_cache, k_rope_cache)
    if slot_ids.dtype != torch.int32 or not slot_ids.is_contiguous():
        raise SlmError("slot_ids must be contiguous int32")
    for t in (kv, k_rope, kv_cache, k_rope_cache):
        if t.dim() != 2 or t.stride(1) != 1 or t.dtype != kv.dtype:
            raise SlmError("mla_set_kv_cache: 2-D tensors of one dtype with contiguous rows")
    if kv.size(0) != slot_ids.numel() or k_rope.size(0) != slot_ids.numel() or kv.size(1) != kv_cache.size(1) or \
            k_rope.size(1) != k_rope_cache.size(1):
        raise SlmError("mla_set_kv_cache: shape mismatch")
    check(_lib.lib().slm_mla_set_kv_cache(slot_ids.data_ptr(), kv.data_ptr(), k_rope.data_ptr(), kv.stride(0),
                                          k_rope.stride(0), kv_cache.data_ptr(), k_rope_cache.data_ptr(),
                                          kv_cache.stride(0), k_rope_cache.stride(0), kv.size(0), kv.size(1),
                                          k_rope.size(1), _dtype_code(kv), _stream()), "slm_mla_set_kv_cache")


def mla_rope_append(q: Optional[torch.Tensor], kv_a: Optional[torch.Tensor], norm_weight: torch.Tensor, eps: float,
                    positions: torch.Tensor, cos_sin: torch.Tensor, interleaved: bool, slot_ids: torch.Tensor,
                    kv_cache: torch.Tensor, k_rope_cache: torch.Tensor, nope_head_dim: int,
                    partials: Optional[DeferredPartials] = None) -> None:
    """The MLA prologue in one launch (slm_hip.h section 18): the latent columns of kv_a [T, latent + rope] are
    RMS-normalised (rms_norm's bits) into kv_cache[slot], its rope columns rotated (apply_rotary_pos_emb's bits)
    into k_rope_cache[slot], and the last `rope` columns of every head of q [T, n_heads, nope + rope] rotated in
    place.  q and kv_a may be column slices of one fused GEMM output; q = None: no query heads.  A negative slot id
    is graph padding: q is rotated, the caches are not written.

    partials (truthy): the fused [q | latent | k_pe] GEMM output was NOT written -- linear / fp8_linear(...,
    defer_reduce=True) left fp32 split-K slabs behind; the kernel sums them itself (the reduce kernel's order and
    rounding: identical bits, one launch less) and WRITES q whole.  kv_a is not used then."""
    L = _lib.lib()
    _require_gpu(q, kv_a, norm_weight, positions, cos_sin, slot_ids, kv_cache, k_rope_cache)
    T = positions.numel()
    latent, rope = kv_cache.size(-1), k_rope_cache.size(-1)
    for t in (positions, slot_ids):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != T:
            raise SlmError("positions / slot_ids must be contiguous int32 [n_tokens]")
    if kv_cache.dim() != 2 or k_rope_cache.dim() != 2 or kv_cache.stride(1) != 1 or k_rope_cache.stride(1) != 1 or \
            kv_cache.size(0) != k_rope_cache.size(0) or kv_cache.dtype != k_rope_cache.dtype:
        raise SlmError("mla_rope_append: caches [n_slots, latent] and [n_slots, rope] of one dtype, rows contiguous")
    dt = kv_cache.dtype
    if norm_weight.dtype != dt or not norm_weight.is_contiguous() or norm_weight.numel() != latent:
        raise SlmError("mla_rope_append: norm_weight must be a contiguous [latent] tensor of the cache dtype")
    is_f32 = 1 if cos_sin.dtype == torch.float32 else 0
    if (not is_f32 and cos_sin.dtype != dt) or not cos_sin.is_contiguous() or cos_sin.size(-1) != rope:
        raise SlmError("cos_sin must be contiguous [max_pos, rope], fp32 or the activation dtype")
    n_heads = 0
    if q is not None:
        if q.dim() != 3 or q.size(0) != T or q.dtype != dt or q.stride(2) != 1 or q.stride(1) != q.size(2) or \
                q.size(2) != nope_head_dim + rope:
            raise SlmError("q must be [n_tokens, n_heads, nope + rope] of the cache dtype, contiguous in its last "
                           "two dims")
        n_heads = q.size(1)
    q_ptr, q_ts = (q.data_ptr(), q.stride(0)) if n_heads else (None, 0)
    tail = (positions.data_ptr(), cos_sin.data_ptr(), is_f32, 1 if interleaved else 0, slot_ids.data_ptr(),
            kv_cache.data_ptr(), k_rope_cache.data_ptr(), kv_cache.stride(0), k_rope_cache.stride(0), T, n_heads,
            int(nope_head_dim), latent, rope, _dtype_code(kv_cache), _stream())
    if partials:
        if not isinstance(partials, DeferredPartials):
            raise SlmError("mla_rope_append(partials=...) takes the handle linear(defer_reduce=True) returned")
        n_cols = n_heads * (nope_head_dim + rope) + latent + rope
        partials.check(kv_cache.device, T * n_cols, "mla_rope_append(partials=...)")
        check(L.slm_mla_rope_append_splitk(partials.ptr, partials.splits, q_ptr, q_ts, norm_weight.data_ptr(),
                                           float(eps), *tail), "slm_mla_rope_append_splitk")
        return
    if kv_a is None or kv_a.dim() != 2 or kv_a.size(0) != T or kv_a.size(1) != latent + rope or kv_a.dtype != dt or \
            kv_a.stride(1) != 1:
        raise SlmError("kv_a must be [n_tokens, latent + rope] of the cache dtype with contiguous rows")
    check(L.slm_mla_rope_append(q_ptr, q_ts, kv_a.data_ptr(), kv_a.stride(0), norm_weight.data_ptr(), float(eps),
                                *tail), "slm_mla_rope_append")
