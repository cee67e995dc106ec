"""Every entry that takes a caller-supplied scratch buffer, run in a buffer of EXACTLY the size its *_workspace_bytes
query reports (include/slm_hip.h: the C-ABI caller allocates that much and may keep anything right behind it).

The Python wrappers get their scratch from kernels._grow, which hands out at least 1 MiB and passes the whole buffer;
here a test-local fixture replaces that one seam.  Each request gets a view of exactly `nbytes` inside a guarded
allocation (tests/scratch_bounds_cases.py: [pre-guard][region][post-guard >= region]), one view per (table, device,
nbytes) for the whole of a run, so that attention's phase 1 and phase 2, or a deferred producer and its consumer,
see the same bytes.  Per case:

  reference  the unpatched wrapper (its values are pinned by the exact tests of each family)
  run A      region 0xFF (NaN in fp32, bf16 and f16), guards 0xA5
  run B      region 0x7F (finite in fp32: 3.4e38), guards 0xFF: an over-read turns into NaN

Both runs must give every output bit for bit as the reference does -- a kernel that reads a partial it never wrote
sees NaN in one run and a huge finite value in the other -- and leave both guards byte for byte as they were.  The
stream-K case gets zeros in its ticket / flag block instead of poison (the host clears it on every call anyway; a
nonzero ticket would send workgroups to slots that do not exist).  Sampling also leaves the rounding slack behind its
[n_rows][max_unique] values untouched."""
import zlib

import numpy as np
import pytest
import torch

from tests import attn_exact_cases as AX
from tests import helpers
from tests import scratch_bounds_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
RUNS = (("A", 0xFF, 0xA5), ("B", 0x7F, 0xFF))


class _Arena:
    """Stands in for kernels._grow during one run: a guarded view of exactly `nbytes` per (table, device, nbytes)"""

    def __init__(self, region_byte, guard_byte, zero_sk_sync):
        self.region_byte, self.guard_byte, self.zero_sk_sync = region_byte, guard_byte, zero_sk_sync
        self.views = {}

    def grow(self, table, nbytes, dev, what):
        from scalellm_amd import kernels
        n = int(nbytes)
        key = (id(table), kernels._dev_key(dev), n)
        if key not in self.views:
            buf = torch.full((S.PRE_GUARD + n + S.post_guard_bytes(n),), self.guard_byte, dtype=torch.uint8,
                             device=dev)
            buf[S.PRE_GUARD:S.PRE_GUARD + n].fill_(self.region_byte)
            if self.zero_sk_sync and n == S.XL_SK_SLOTS + S.XL_SK_SYNC:
                buf[S.PRE_GUARD + S.XL_SK_SLOTS:S.PRE_GUARD + n].zero_()
            self.views[key] = (buf, n, what)
        buf, _, _ = self.views[key]
        return buf[S.PRE_GUARD:S.PRE_GUARD + n]


@pytest.fixture
def exact_scratch(monkeypatch):
    """exact_scratch(fn, region_byte, guard_byte, zero_sk_sync) -> (fn's outputs, arena): fn runs with kernels._grow
    replaced by a fresh _Arena; conftest and the module-level tables stay untouched"""
    from scalellm_amd import kernels

    def run(fn, region_byte, guard_byte, zero_sk_sync=False):
        arena = _Arena(region_byte, guard_byte, zero_sk_sync)
        with monkeypatch.context() as m:
            m.setattr(kernels, "_grow", arena.grow)
            out = fn()
            torch.cuda.synchronize()
        return out, arena
    return run


def _gen(name):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(name.encode()))


def _nan(*shape, dtype=BF16):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


# ---- attention and MLA --------------------------------------------------------------------------------------------------
def _attn_inputs(case):
    c = case.spec["attn"]
    lay = AX.layout(c)
    K, V = AX.caches(c, "spike")
    up = lambda a, dt=BF16: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dt)  # noqa: E731
    idx = tuple(up(x, torch.int32) for x in (lay.q_cu, lay.kv_cu, lay.bt, lay.bcu))
    T, D = S.attn_n_tokens(c), c.head_dim
    Dk = D + (AX.MLA_ROPE if c.kind == "mla" else 0)
    q = torch.randn(T, c.heads, Dk, device=DEV, generator=_gen(case.name)).to(BF16)
    if c.kind == "mla":
        return dict(q=q[..., :D].contiguous(), qr=q[..., D:].contiguous(), kv=up(V[:, 0]), kr=up(K[:, 0, D:]), idx=idx)
    return dict(q=q, k=up(K), v=up(V), idx=idx)


def _attn_run(case, x):
    from scalellm_amd import kernels
    c = case.spec["attn"]
    max_q = max(max(c.q_lens), 1)
    max_kv = c.max_kv_hint if c.max_kv_hint is not None else max(c.kv_lens)
    out = _nan(*x["q"].shape[:2], c.head_dim)
    if c.kind == "mla":
        kernels.mla_paged_kv(out, x["q"], x["qr"], x["kv"], x["kr"], *x["idx"], c.block, max_q, max_kv,
                             AX.sm_scale_of(c), num_splits=c.num_splits)
        return dict(out=out)
    args = (out, x["q"], x["k"], x["v"], *x["idx"], None, c.block, max_q, max_kv, AX.sm_scale_of(c), c.softcap,
            c.window, c.num_splits)
    if case.spec["phased"]:
        kernels.paged_kv_varlen_mha(*args, phase=1)
        kernels.paged_kv_varlen_mha(*args, phase=2)
    else:
        kernels.paged_kv_varlen_mha(*args)
    return dict(out=out)


# ---- int4 / int8 GEMMs --------------------------------------------------------------------------------------------------
def _w4_packed(s, seed):
    if s["bits8"]:
        return helpers.pack_case8(helpers.make_quant8_case(seed, s["K"], s["N"], s["gs"], s["fmt"], "bf16"), "bf16")
    q = helpers.make_quant_case(seed, s["K"], s["N"], s["gs"], s["fmt"], "bf16", act_order=s["act"])
    return helpers.pack_case(q, "bf16")


def _w4_inputs(case):
    s, g = case.spec, _gen(case.name)
    M, N, K = s["M"], s["N"], s["K"]
    x = dict(w=_w4_packed(s, zlib.crc32(case.name.encode()) % 100000), a=torch.randn(M, K, device=DEV, generator=g).to(BF16))
    x["bias"] = (0.1 * torch.randn(N, device=DEV, generator=g)).to(BF16) if s["bias"] else None
    if s["consumer"] is not None:
        x["nw"] = (1 + 0.1 * torch.randn(N, device=DEV, generator=g)).to(BF16)
        x["res"] = torch.randn(M, N, device=DEV, generator=g).to(BF16)
    if s["consumer"] == "gemv_norm":      # a second [K = N, N] layer whose norm prologue reads the first one's slabs
        x["w2"] = _w4_packed(dict(s, K=N), zlib.crc32(case.name.encode()) % 100000 + 1)
    return x


def _w4_run(case, x):
    from scalellm_amd import kernels
    s = case.spec
    M, N = s["M"], s["N"]
    c = _nan(M, N)
    if s["consumer"] is None:
        assert not kernels.gptq_gemm(x["a"], x["w"], c, x["bias"])
        return dict(c=c)
    h = kernels.gptq_gemm(x["a"], x["w"], c, defer_reduce=True)
    assert int(h) >= 2 and bool(torch.isnan(c).all()), "the call was meant to defer its reduction"
    if s["consumer"] == "rms_norm":
        out, res = _nan(M, N), x["res"].clone()
        kernels.rms_norm(out, c, x["nw"], 1e-5, res, partials=h)
        return dict(out=out, res=res)
    # gemv_norm: test_gemv_norm_gpu's fused chain -- the prologue reads slot 0 and leaves its own slabs in slot 1
    y, res, res_out = _nan(M, N), x["res"].clone(), _nan(M, N)
    h2 = kernels.gptq_gemm(c, x["w2"], y, defer_reduce=True,
                           norm=kernels.NormPrologue(x["nw"], 1e-5, residual=res, residual_out=res_out, partials=h))
    assert h2 and h2.slot == 1
    final = _nan(M, N)
    kernels.rms_norm(final, y, x["nw"], 1e-5, partials=h2)
    return dict(final=final, res_out=res_out, res=res)


# ---- dense / fp8 linears and their deferred consumers ---------------------------------------------------------------------
def _linear_inputs(case):
    from scalellm_amd import kernels
    s, g = case.spec, _gen(case.name)
    M, N, K = s["M"], s["N"], s["K"]
    w = (0.05 * torch.randn(N, K, device=DEV, generator=g)).to(BF16)
    x = dict(a=torch.randn(M, K, device=DEV, generator=g).to(BF16), bias=(0.1 * torch.randn(N, device=DEV, generator=g)).to(BF16))
    if s["fp8"]:
        x["w8"], x["scale"] = kernels.quantize_fp8_weight(w)
    else:
        x["w"] = w
    x["nw"] = (1 + 0.1 * torch.randn(N, device=DEV, generator=g)).to(BF16)
    x["res"] = torch.randn(M, N, device=DEV, generator=g).to(BF16)
    x["post"] = (0.1 * torch.randn(N, device=DEV, generator=g)).to(BF16)
    x["pos"] = torch.arange(3, 3 + M, dtype=torch.int32, device=DEV)
    x["slots"] = torch.arange(5, 5 + M, dtype=torch.int32, device=DEV)
    return x


def _linear(x, c, bias=None, defer=False):
    from scalellm_amd import kernels
    if "w8" in x:
        return kernels.fp8_linear(x["a"], x["w8"], x["scale"], c, bias, defer_reduce=defer)
    return kernels.linear(x["a"], x["w"], c, bias, defer_reduce=defer)


def _cos_sin(dim):
    from scalellm_amd.layers import HipAttnHandler
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, dim, 2, dtype=torch.float32, device=DEV) / dim))
    return HipAttnHandler.build_cos_sin(dim, 64, inv_freq)


def _linear_run(case, x):
    from scalellm_amd import kernels
    s = case.spec
    M, N = s["M"], s["N"]
    c = _nan(M, N)
    assert not _linear(x, c, x["bias"])                       # split, reduced with the bias: the shared workspace
    buf = _nan(M, N)
    h = _linear(x, buf, defer=True)                           # slabs in the deferred buffer
    assert int(h) == s["split"]
    got = dict(c=c)
    consumer = s["consumer"]
    if consumer == "rms_norm":
        out, res = _nan(M, N), x["res"].clone()
        kernels.rms_norm(out, buf, x["nw"], 1e-5, residual=res, partials=h)
        got.update(out=out, res=res)
    elif consumer == "gemma":
        out, res = _nan(M, N), x["res"].clone()
        kernels.gemma_sandwich_norm(out, buf, x["post"], res, x["nw"], 1e-6, partials=h)
        got.update(out=out, res=res)
    elif consumer in ("rope", "qk_norm"):
        sh = S.ROPE_SHAPE if consumer == "rope" else S.QKN_SHAPE
        H, HKV, D = sh["H"], sh["HKV"], sh["D"]
        assert (sh["T"], (H + 2 * HKV) * D) == (M, N)
        kc, vc = _nan(32, HKV, D), _nan(32, HKV, D)
        q = buf[:, :H * D].view(M, H, D)
        k = buf[:, H * D:(H + HKV) * D].view(M, HKV, D)
        v = buf[:, (H + HKV) * D:].view(M, HKV, D)
        if consumer == "rope":
            kernels.apply_rotary_pos_emb(q, k, x["pos"], _cos_sin(D), D, False, value=v, slot_ids=x["slots"],
                                         key_cache=kc, value_cache=vc, partials=h)
        else:
            kernels.qk_norm_rope_kv_append(q, k, v, x["nw"][:D].contiguous(), x["nw"][D:2 * D].contiguous(), 1e-6,
                                           x["pos"], _cos_sin(D), False, slot_ids=x["slots"], key_cache=kc,
                                           value_cache=vc, partials=h)
        got.update(qkv=buf, kc=kc, vc=vc)
    else:                                                     # mla_prologue: [q | latent | k_pe] columns
        sh = S.MLA_PRO_SHAPE
        H, NOPE, LAT, R = sh["H"], sh["NOPE"], sh["LATENT"], sh["ROPE"]
        assert (sh["T"], H * (NOPE + R) + LAT + R) == (M, N)
        q = buf[:, :H * (NOPE + R)].view(M, H, NOPE + R)
        kvc, krc = _nan(32, LAT), _nan(32, R)
        kernels.mla_rope_append(q, None, x["nw"][:LAT].contiguous(), 1e-6, x["pos"], _cos_sin(R), False, x["slots"],
                                kvc, krc, NOPE, partials=h)
        got.update(q=q.contiguous(), kvc=kvc, krc=krc)
    return got


# ---- sampling, rejection, router ------------------------------------------------------------------------------------------
def _sampling_inputs(case):
    s, g = case.spec, _gen(case.name)
    n, mu, V = s["n_rows"], s["max_unique"], s["vocab"]
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    ids = np.stack([rng.choice(V, size=mu, replace=False) for _ in range(n)]).astype(np.int64)
    lens = rng.integers(0, mu + 1, size=n).astype(np.int32)
    lens[-1] = mu                                             # the last row fills its whole [max_unique] row
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return dict(
        logits=(3 * torch.randn(n, V, device=DEV, generator=g)).to(BF16),
        kw=dict(frequency_penalties=t(rng.uniform(0.1, 0.5, n).astype(np.float32)),
                presence_penalties=t(rng.uniform(0.1, 0.5, n).astype(np.float32)),
                repetition_penalties=t(rng.uniform(1.1, 1.5, n).astype(np.float32)),
                temperatures=t(rng.uniform(0.7, 1.3, n).astype(np.float32)),
                top_k=t(rng.integers(5, 200, n).astype(np.int64)),
                top_p=t(rng.uniform(0.8, 0.95, n).astype(np.float32)),
                unique_token_ids=t(ids), unique_token_counts=t(rng.integers(1, 6, size=(n, mu)).astype(np.int32)),
                unique_token_lens=t(lens)))


def _sampling_run(case, x):
    from scalellm_amd import kernels
    n, V = case.spec["n_rows"], case.spec["vocab"]
    if case.entry == "slm_logits_process":
        processed = _nan(n, V)
        kernels.logits_process(x["logits"], processed, **x["kw"])
        return dict(processed=processed)
    nxt = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    probs, lp = _nan(n, V, dtype=torch.float32), _nan(n, dtype=torch.float32)
    kernels.sample(x["logits"], nxt, probs=probs, logprobs=lp, do_sample=torch.arange(n, device=DEV) % 2 == 0,
                   seeds=torch.arange(11, 11 + n, device=DEV), positions=torch.arange(n, dtype=torch.int32, device=DEV),
                   **x["kw"])
    return dict(next_tokens=nxt, probs=probs, logprobs=lp)


def _rejection_inputs(case):
    s, g = case.spec, _gen(case.name)
    n, k, V = s["n_seqs"], s["k"], s["vocab"]
    draft_logits = torch.randn(n, k, V, device=DEV, generator=g)
    target = (draft_logits.repeat(1, 2, 1)[:, :k + 1] + 0.5 * torch.randn(n, k + 1, V, device=DEV, generator=g)).to(BF16)
    return dict(draft_ids=torch.randint(0, V, (n, k), device=DEV, generator=g, dtype=torch.int32),
                draft_probs=torch.softmax(draft_logits, -1).contiguous(), target=target,
                bonus=torch.randint(0, V, (n,), device=DEV, generator=g, dtype=torch.int32))


def _rejection_run(case, x):
    from scalellm_amd import kernels
    n, k = case.spec["n_seqs"], case.spec["k"]
    acc = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lp = _nan(n, k + 1, dtype=torch.float32) if case.spec["logprobs"] else None
    nxt = kernels.rejection_sample(x["draft_ids"], x["draft_probs"], x["target"], x["bonus"],
                                   do_sample=torch.arange(n, device=DEV) % 3 != 1, seeds=torch.arange(5, 5 + n, device=DEV),
                                   positions=torch.arange(n, dtype=torch.int32, device=DEV), accepted_lens=acc, logprobs=lp)
    got = dict(next_tokens=nxt, accepted_lens=acc)
    if lp is not None:
        got["logprobs"] = lp
    return got


def _records(case, region):
    """the 16-byte per-row records launch 1 of rejection_sample leaves in its workspace for launch 2 (rejection.hip):
    rows [0, k) of every sequence, and row k (the bonus row) when logprobs are asked for"""
    n, k = case.spec["n_seqs"], case.spec["k"]
    rows = k + 1 if case.spec["logprobs"] else k
    return region[:n * (k + 1) * 16].view(n, k + 1, 16)[:, :rows]


def _router_inputs(case):
    s, g = case.spec, _gen(case.name)
    return dict(x=torch.randn(s["T"], s["H"], device=DEV, generator=g).to(BF16),
                w=torch.randn(s["E"], s["H"], device=DEV, generator=g).to(BF16))


def _router_run(case, x):
    from scalellm_amd import kernels
    w, i = kernels.moe_router(x["x"], x["w"], case.spec["topk"])
    return dict(weights=w, indices=i)


FAMILIES = {"attn": (_attn_inputs, _attn_run), "mla": (_attn_inputs, _attn_run), "w4": (_w4_inputs, _w4_run),
            "linear": (_linear_inputs, _linear_run), "sampling": (_sampling_inputs, _sampling_run),
            "rejection": (_rejection_inputs, _rejection_run), "router": (_router_inputs, _router_run)}


def _bytes(t):
    return t.detach().contiguous().view(-1).view(torch.uint8).cpu()


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_runs_in_exactly_its_reported_workspace(case, exact_scratch):
    from scalellm_amd import kernels
    make, run = FAMILIES[case.family]
    stream_k = case.spec.get("kernel") == "XL_SK"
    with kernels.tuning(**case.knobs):
        need = S.workspace_bytes(case)
        x = make(case)
        ref = {k: _bytes(v) for k, v in run(case, x).items()}
        torch.cuda.synchronize()
        if case.family == "rejection":
            ref["records"] = _bytes(_records(case, kernels._rejection_ws[kernels._dev_key(torch.device(DEV))]))
        for tag, region_byte, guard_byte in RUNS:
            got, arena = exact_scratch(lambda: run(case, x), region_byte, guard_byte, stream_k)
            sizes = sorted(n for _, n, _ in arena.views.values())
            if case.family == "router":
                assert need == 0 and not sizes, (case.name, "the router reports no workspace and must ask for none")
            else:
                want = set(need) if isinstance(need, tuple) else {need}
                assert sizes and set(sizes) <= want, (case.name, "scratch requests other than the reported sizes",
                                                      sizes, need)
            for buf, n, what in arena.views.values():
                bad = S.guard_violations(buf, n, guard_byte)
                assert not bad, f"{case.name} run {tag}: {what} of {n} bytes: guard bytes changed at offsets {bad}"
                # the kernels did work in the handed-out region (the stream-K ticket block was zeroed by the test)
                body = buf[S.PRE_GUARD:S.PRE_GUARD + (S.XL_SK_SLOTS if stream_k else n)]
                assert bool((body != region_byte).any()), f"{case.name} run {tag}: nothing was written to the {what}"
                if case.family == "sampling":
                    used = case.spec["n_rows"] * case.spec["max_unique"] * 4
                    slack = buf[S.PRE_GUARD + used:S.PRE_GUARD + n]
                    assert bool((slack == region_byte).all()), \
                        f"{case.name} run {tag}: the rounding slack behind byte {used} of the {n}-byte workspace changed"
                if case.family == "rejection":
                    got["records"] = _records(case, buf[S.PRE_GUARD:S.PRE_GUARD + n])
            assert set(got) == set(ref)
            for k, v in got.items():
                b = _bytes(v)
                diff = torch.nonzero(b != ref[k]).flatten()
                assert diff.numel() == 0, (f"{case.name} run {tag} (region 0x{region_byte:02X}): output {k} differs "
                                           f"from the reference in {diff.numel()} bytes, first at byte {int(diff[0])}")
