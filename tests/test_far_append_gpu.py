"""KV append into caches whose rows lie more than 2 GiB and more than 4 GiB from the cache pointer: set_kv_cache,
mla_set_kv_cache, rope_kv_append (vector kernel, scalar kernel, split-K slab form), qk_norm_rope_kv_append (plain,
slabs) and mla_rope_append (plain, slabs), each with one token per zone of tests/far_arena.py (the last row of the
view among them) plus one slot id -1 (set_kv_cache excepted: it has no padding rows, a negative id is the caller's
error).  The K-region view takes the key / latent cache, the V-region view the value / RoPE-key cache; the latter has
128-byte rows in the MLA cases and reaches 2^31 but not 2^32.

Bars, all bit for bit: the far rows equal the rows the same call, on the same inputs, writes into a small compact
cache; q / k written in place equal the compact run's; and after every launch the arena outside the six rows of each
view still holds the poison (far_arena.untouched), the pad in front of region K included.

The address arithmetic the far zones exercise (slot is an int32 id widened to int64 before the product):
  kv_cache.hip   key_cache + slot * (int64_t)row_bytes
  mla.hip        kv_cache + slot * kv_ss_b, k_rope_cache + slot * kr_ss_b  (int64 slot and strides)
  glue.hip       key_cache + slot * row + h * head_dim (+ d), value_cache + slot * row + i * 8 (vector: st4 / u32x4;
                 scalar: element stores), slot = (int64_t)slot_ids[tok]
  qk_norm.hip    p.kc + slot * row + hh * D + j * 8, p.vc + slot * row + i * 8
  mla_glue.hip   p.kvc + slot * p.kvc_ss + lane * 8, p.krc + slot * p.krc_ss
Shapes: the smallest of glue_ref.ROPE (V1, S3), qk_norm_ref.CASES (d64-h1) and mla_glue_ref.CASES (h1) that reach each
kernel form, with 7 tokens so that every zone gets one.  tests/test_far_offsets_cpu.py shows that each of the three
32-bit slips breaks the row equality."""
import numpy as np
import pytest
import torch

from tests import far_arena as F
from tests import glue_ref as ref
from tests import mla_glue_ref as mref
from tests import qk_norm_ref as qref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
NEG = 3                                   # the token whose slot id is -1
COMPACT_SLOTS = 8
COMPACT = np.array([5, 0, 7, 2, 6, 3])    # compact slots of the six far rows; 1 and 4 stay poison


@pytest.fixture(scope="module")
def arena():
    torch.cuda.reset_peak_memory_stats()
    holder = [F.allocate()]
    yield holder[0]
    holder.clear()
    torch.cuda.empty_cache()
    print(f"FAR-ARENA append: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _poison(bits, *shape):
    return torch.full(shape, F.POISON_BITS[bits], dtype=torch.int16, device=DEV).view(TDT[bits])


def _ids(slots, with_neg):
    s = np.insert(np.asarray(slots, np.int64), NEG, -1) if with_neg else np.asarray(slots, np.int64)
    return torch.from_numpy(s.astype(np.int32)).to(DEV)


def _table(t64):
    return torch.from_numpy(np.asarray(t64, np.float32)).to(DEV)


# every runner: (bits, key-side cache, value-side cache, slot ids [T]) -> the tensors the launch wrote in place
def _set_kv_cache(bits, kc, vc, slots):
    from scalellm_amd import kernels
    k, v = (_randn(s, 6, 2, 64).to(TDT[bits]).to(DEV) for s in (1, 2))
    kernels.set_kv_cache(slots, k, v, kc, vc)
    return []


def _mla_set_kv_cache(bits, kc, vc, slots):
    from scalellm_amd import kernels
    kv, kr = _randn(3, 7, 128).to(TDT[bits]).to(DEV), _randn(4, 7, 64).to(TDT[bits]).to(DEV)
    kernels.mla_set_kv_cache(slots, kv, kr, kc, vc)
    return []


def _rope(form):
    nh, nkv, D = 4, 2, 64
    rot = {"vector": 32, "scalar": 64, "slabs": 32}[form]
    n_cols = (nh + 2 * nkv) * D

    def run(bits, kc, vc, slots):
        from scalellm_amd import kernels
        dt = TDT[bits]
        row = _randn(5, 7, n_cols)
        pad = 2 if form == "scalar" else 0                  # S3: token stride % 4 = 2 keeps the call off the vector kernel
        buf = torch.zeros(7, n_cols + pad, dtype=dt, device=DEV)
        buf[:, :n_cols] = row.to(dt).to(DEV)
        q = buf[:, :nh * D].view(7, nh, D) if form != "vector" else buf[:, :nh * D].contiguous().view(7, nh, D)
        k = buf[:, nh * D:(nh + nkv) * D].view(7, nkv, D) if form != "vector" else \
            buf[:, nh * D:(nh + nkv) * D].contiguous().view(7, nkv, D)
        v = buf[:, (nh + nkv) * D:n_cols].view(7, nkv, D) if form != "vector" else \
            buf[:, (nh + nkv) * D:n_cols].contiguous().view(7, nkv, D)
        want = "scalar" if form == "scalar" else "vector"
        assert ref.rope_dispatch(nh, nkv, D, rot, q.stride(0), k.stride(0), v.stride(0), True)[0] == want
        pos = torch.tensor([36, 0, 5, 17, 5, 30, 1], dtype=torch.int32, device=DEV)
        tab = _table(ref.real_rope_table(rot, "f32", bits))
        partials = None
        if form == "slabs":
            slabs = (_randn(6, 2, 7, n_cols) / 2 ** 0.5).to(DEV)
            partials = kernels.DeferredPartials.from_slabs(slabs)
            buf.fill_(0)                                    # q, k, v are outputs in this form
        kernels.apply_rotary_pos_emb(q, k, pos, tab, rot, False, value=v, slot_ids=slots, key_cache=kc, value_cache=vc,
                                     partials=partials)
        return [q, k, v]
    return run


def _qk_norm(slab_form):
    H, KV, D = 1, 1, 64

    def run(bits, kc, vc, slots):
        from scalellm_amd import kernels
        dt = TDT[bits]
        q, k, v = (_randn(s, 7, n, D).to(dt).to(DEV) for s, n in ((7, H), (8, KV), (9, KV)))
        qw, kw = ((1 + 0.25 * _randn(s, D)).to(dt).to(DEV) for s in (10, 11))
        pos = torch.tensor([40, 0, 5, 17, 5, 30, 1], dtype=torch.int32, device=DEV)
        tab = _table(qref.table("f32", bits, D))
        partials = None
        if slab_form:
            slabs = (_randn(12, 2, 7, (H + 2 * KV) * D) / 2 ** 0.5).to(DEV)
            partials = kernels.DeferredPartials.from_slabs(slabs)
        kernels.qk_norm_rope_kv_append(q, k, v, qw, kw, qref.EPS, pos, tab, True, slot_ids=slots, key_cache=kc,
                                       value_cache=vc, partials=partials)
        return [q, k, v]
    return run


def _mla_rope(slab_form):
    latent, nope, heads, rope = 128, 32, 1, mref.ROPE

    def run(bits, kc, vc, slots):
        from scalellm_amd import kernels
        dt = TDT[bits]
        q = _randn(13, 7, heads, nope + rope).to(dt).to(DEV)
        kv_a = _randn(14, 7, latent + rope).to(dt).to(DEV)
        w = (1 + 0.25 * _randn(15, latent)).to(dt).to(DEV)
        pos = torch.tensor([40, 0, 5, 17, 5, 30, 1], dtype=torch.int32, device=DEV)
        tab = _table(mref.table("f32", bits))
        partials = None
        if slab_form:
            slabs = (_randn(16, 2, 7, heads * (nope + rope) + latent + rope) / 2 ** 0.5).to(DEV)
            partials = kernels.DeferredPartials.from_slabs(slabs)
        kernels.mla_rope_append(q, None if slab_form else kv_a, w, mref.EPS, pos, tab, True, slots, kc, vc, nope,
                                partials=partials)
        return [q]
    return run


# name (a key of far_arena.ROW_CASES) -> (runner, shape of a key-side row, shape of a value-side row, has a -1 token)
CASES = {
    "set_kv_cache": (_set_kv_cache, (2, 64), (2, 64), False),
    "mla_set_kv_cache": (_mla_set_kv_cache, (128,), (64,), True),
    "rope_kv_append vector": (_rope("vector"), (2, 64), (2, 64), True),
    "rope_kv_append scalar": (_rope("scalar"), (2, 64), (2, 64), True),
    "rope_kv_append slabs": (_rope("slabs"), (2, 64), (2, 64), True),
    "qk_norm_rope_kv_append": (_qk_norm(False), (1, 64), (1, 64), True),
    "qk_norm_rope_kv_append slabs": (_qk_norm(True), (1, 64), (1, 64), True),
    "mla_rope_append": (_mla_rope(False), (128,), (64,), True),
    "mla_rope_append slabs": (_mla_rope(True), (128,), (64,), True),
}
assert set(CASES) == {n for n, _, _ in F.APPEND}


@pytest.mark.parametrize("bits", ref.BITS)
@pytest.mark.parametrize("name", list(CASES), ids=[n.replace(" ", "-") for n in CASES])
def test_far_append(name, bits, arena):
    run, k_shape, v_shape, with_neg = CASES[name]
    k_row, v_row = F.ROW_CASES[name]
    assert (int(np.prod(k_shape)) * 2, int(np.prod(v_shape)) * 2) == (k_row, v_row)
    far, _ = F.case_rows(name)
    F.refill(arena, bits)
    kc = F.view(arena, F.K_BASE, TDT[bits], *k_shape)
    vc = F.view(arena, F.V_BASE, TDT[bits], *v_shape)[:F.REGION // k_row]      # one slot count for both views
    ck, cv = _poison(bits, COMPACT_SLOTS, *k_shape), _poison(bits, COMPACT_SLOTS, *v_shape)
    outs_far = run(bits, kc, vc, _ids(far, with_neg))
    torch.cuda.synchronize()
    assert F.untouched(arena, F.rows_written(name), bits), (name, "wrote outside the rows of its slot ids")
    outs_near = run(bits, ck, cv, _ids(COMPACT, with_neg))
    torch.cuda.synchronize()
    for a, b in zip(outs_far, outs_near):
        assert np.array_equal(_bits(a), _bits(b)), (name, "in-place q / k / v differ from the compact run")
    poison = F.POISON_BITS[bits]
    for what, fc, cc in (("key side", kc, ck), ("value side", vc, cv)):
        near = _bits(cc)
        assert (near[[1, 4]] == poison).all() and not (near[COMPACT] == poison).all(axis=tuple(range(1, near.ndim))).any()
        for z, (f, c) in enumerate(zip(far, COMPACT)):
            got = _bits(fc[int(f):int(f) + 1])[0]
            assert np.array_equal(got, near[c]), (name, bits, what, "zone", F.ZONES[5 - z], "slot", int(f))
