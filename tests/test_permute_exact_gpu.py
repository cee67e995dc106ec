"""Exact GPU tests of the MoE token permutation kernels (include/slm_hip.h section 14; csrc/permute.hip): both maps
integer for integer against numpy, the permuted rows bit for bit, the un-permute at 0 ulp where the result is
representable and within the fp32-accumulation bound elsewhere, graph replay, and the C++ shim."""
import numpy as np
import pytest
import torch

from . import permute_ref as ref
from .permute_ref import as64, torch_dtype

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = {"bf16": 0x7b7b, "f16": 0x7b7b, "f32": 0x7b7b7b7b}
ROW_DIMS = {"bf16": (8, 16, 64, 520, 4104), "f16": (8, 16, 64, 520, 4104), "f32": (4, 16, 64)}


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


# ---- maps ------------------------------------------------------------------------------------------------------------
def test_index_maps_equal_numpy():
    from scalellm_amd import kernels
    for case in ref.INDEX_CASES:
        name, T, k, E, _ = case
        ids = ref.index_case(*case)
        want_map, want_counts = ref.index_map(ids, E)
        got_map, got_counts = kernels.permute_index_map(_i32(ids), E, count=True)
        assert got_map.shape == (k, T) and np.array_equal(got_map.cpu().numpy(), want_map), name
        assert np.array_equal(got_counts.cpu().numpy(), want_counts), name
        again, _ = kernels.permute_index_map(_i32(ids), E)             # without the counts; repeats are identical
        assert torch.equal(again, got_map), name
        # told only the upper bound of the expert range (the shim's call): the same rows
        if int(ids.max()) < E and int(ids.min()) >= 0:
            wide, _ = kernels.permute_index_map(_i32(ids))
            assert torch.equal(wide, got_map), name


def test_mask_maps_equal_numpy():
    from scalellm_amd import kernels
    for case in ref.MASK_CASES:
        name, T, E, _ = case
        mask = ref.mask_case(*case)
        want_map, want_counts = ref.mask_map(mask)
        n_perm = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        m = torch.from_numpy(mask).to(DEV)
        got_map, got_counts = kernels.permute_mask_map(m, n_permuted=n_perm, count=True)
        assert got_map.shape == (E, T) and np.array_equal(got_map.cpu().numpy(), want_map), name
        assert np.array_equal(got_counts.cpu().numpy(), want_counts), name
        assert int(n_perm[0]) == int(mask.sum()), name
        # a mask whose base is not 16-byte aligned (the count then goes byte by byte), and bytes other than 1
        shifted = torch.zeros(T * E + 3, dtype=torch.uint8, device=DEV)[3:].view(T, E)
        shifted.copy_(m.to(torch.uint8) * 200)
        assert shifted.data_ptr() % 16 != 0
        again, _ = kernels.permute_mask_map(shifted)
        assert torch.equal(again, got_map), name


# ---- permuted rows -----------------------------------------------------------------------------------------------------
def _permute_check(kernels, bits, T, dim, row_map, rows, what):
    """scatter bit-pattern rows through row_map [n_maps, T] into a sentinel-filled buffer of `rows` rows + a guard"""
    it = ref.int_dtype(bits)
    tok = ref.bit_tokens(T, dim, bits)
    buf = torch.full((rows + 1, dim), SENTINEL[bits], dtype=it)
    want = ref.permute_rows(tok.numpy(), row_map, buf[:rows].numpy())
    dbuf = buf.to(DEV)
    kernels.permute_rows(tok.to(DEV).view(torch_dtype(bits)), _i32(row_map), dbuf[:rows].view(torch_dtype(bits)))
    got = dbuf.cpu()
    assert np.array_equal(got[:rows].numpy(), want), what
    assert bool((got[rows] == SENTINEL[bits]).all()), what               # the guard row
    return dbuf[:rows].view(torch_dtype(bits))


@pytest.mark.parametrize("bits", ref.BITS)
def test_permuted_rows_equal_the_gather_bit_for_bit(bits):
    from scalellm_amd import kernels
    rng = np.random.default_rng(1)
    shapes = [(1, 1, 1), (2, 2, 4), (16, 4, 64), (63, 3, 8), (64, 8, 256), (65, 1, 4), (257, 2, 8)]
    for n, (T, k, E) in enumerate(shapes):
        dim = ROW_DIMS[bits][n % len(ROW_DIMS[bits])]
        ids = ref.distinct_ids(rng, T, k, E)
        imap, counts = ref.index_map(ids, E)
        by_index = _permute_check(kernels, bits, T, dim, imap, T * k, ("index", T, k, E, dim))
        mmap, _ = ref.mask_map(ref.ids_to_mask(ids, E))
        by_mask = _permute_check(kernels, bits, T, dim, mmap, T * k, ("mask", T, k, E, dim))
        assert torch.equal(by_index.view(ref.int_dtype(bits)), by_mask.view(ref.int_dtype(bits)))   # distinct ids
    for dim in ROW_DIMS[bits]:                                          # every dim, more than one segment at 4104
        ids = ref.distinct_ids(rng, 5, 2, 8)
        _permute_check(kernels, bits, 5, dim, ref.index_map(ids, 8)[0], 10, ("dims", dim))


@pytest.mark.parametrize("bits", ref.BITS)
def test_unmapped_rows_keep_the_sentinel(bits):
    from scalellm_amd import kernels
    dim = ROW_DIMS[bits][2]
    ids = ref.index_case("out_of_range", 65, 3, 8, "foreign")
    imap, counts = ref.index_map(ids, 8)
    n = int(counts.sum())
    assert 0 < n < 65 * 3
    _permute_check(kernels, bits, 65, dim, imap, 65 * 3, "rows past the mapped count")   # [n, 195) stay
    _permute_check(kernels, bits, 65, dim, imap, n - 7, "entries >= permuted_rows")      # the last 7 are dropped
    _permute_check(kernels, bits, 65, dim, imap, 0, "permuted_rows = 0")
    mask = ref.mask_case("irregular", 65, 8, None)
    _permute_check(kernels, bits, 65, dim, ref.mask_map(mask)[0], 65 * 8, "irregular mask")
    # garbage in the map: negative and huge entries store nothing
    wild = imap.copy()
    wild[0, :5] = [-2, -(1 << 31), (1 << 31) - 1, 65 * 3, 65 * 3 + 1]
    _permute_check(kernels, bits, 65, dim, wild, 65 * 3, "wild entries")


# ---- un-permute ----------------------------------------------------------------------------------------------------------
def _roundtrip(kernels, bits, T, k, E, dim, probs_dtype, form, rng):
    dt = torch_dtype(bits)
    x = ref.rounded(rng.standard_normal((T, dim)), bits).to(DEV)
    ids = ref.distinct_ids(rng, T, k, E)
    if form == "index":
        permuted, rmap = kernels.permute_with_index_map(x, _i32(ids), E)
        probs = torch.full((T, k), 1.0 / k, dtype=probs_dtype, device=DEV)
        out = kernels.unpermute_with_index_map(permuted, rmap, probs)
    else:
        mask = torch.from_numpy(ref.ids_to_mask(ids, E)).to(DEV)
        permuted, rmap = kernels.permute_with_mask_map(x, mask, k)
        probs = (mask.to(torch.float32) / k).to(probs_dtype)
        out = kernels.unpermute_with_mask_map(permuted, rmap, probs)
    assert out.dtype == dt and out.shape == x.shape
    return x, out


@pytest.mark.parametrize("bits", ref.BITS)
def test_round_trip_with_probs_one_over_k_is_exact(bits):
    """fp32 probs 1 / k: the fp32 chain fma(p, x, acc) perturbs the token by less than 2^-22 relative (k roundings of
    the running sum and |k * fl(1 / k) - 1| <= 2^-24, against partial sums no larger than the token).  That is far
    inside half an ulp of f16 / bf16 (2^-12 / 2^-9), so the one rounding returns the token bit for bit for EVERY k.
    For fp32 rows half an ulp is 2^-24 itself and the partial sums j * x / k (3 x / 4, say) need more than 24 bits:
    exact only for k = 1, 2; the other k are held to the bound of the random-data test below with sum |p x| = |x| and
    the k live slots: 1 ulp + k * 2^-23 * |x| <= (k + 1) * 2^-23 * |x|.
    Probabilities of the rows' own 16-bit dtype: 1 / k is exact for the powers of two, same argument."""
    from scalellm_amd import kernels
    rng = np.random.default_rng(2)
    dt = torch_dtype(bits)
    for k, T, E in ((1, 1, 1), (2, 2, 4), (3, 63, 8), (4, 16, 64), (8, 65, 256), (3, 257, 4), (8, 64, 8)):
        dim = ROW_DIMS[bits][k % len(ROW_DIMS[bits])]
        for form in ("index", "mask"):
            x, out = _roundtrip(kernels, bits, T, k, E, dim, torch.float32, form, rng)
            if bits != "f32" or k <= 2:
                assert torch.equal(out, x), (form, k, T, E, dim)
            else:
                assert bool(((out - x).abs() <= (k + 1) * 2.0 ** -23 * x.abs()).all()), (form, k, T, E, dim)
            if k & (k - 1) == 0 and (bits != "f32" or k <= 2):
                x, out = _roundtrip(kernels, bits, T, k, E, dim, dt, form, rng)
                assert torch.equal(out, x), (form, k, T, E, dim, "probs in the rows' dtype")


@pytest.mark.parametrize("bits", ref.BITS)
def test_integer_rows_with_power_of_two_probabilities_are_exact(bits):
    """|x| <= 4, p in {1/2, 1}, at most 8 terms: every partial sum is a multiple of 1/2 below 32, exact in fp32 in
    any order and representable in bf16's 8 significant bits, so the result must be the sum, bit for bit"""
    from scalellm_amd import kernels
    rng = np.random.default_rng(3)
    for T, k, E in ((5, 8, 256), (65, 3, 8), (16, 2, 4)):
        dim = ROW_DIMS[bits][1]
        ids = ref.distinct_ids(rng, T, k, E)
        imap, counts = ref.index_map(ids, E)
        rows = ref.rounded(rng.integers(-4, 5, size=(T * k, dim)), bits)
        probs = 2.0 ** rng.integers(-1, 1, size=(T, k))
        want, _ = ref.unpermute64(as64(rows), imap, probs)
        assert torch.equal(ref.rounded(want, bits).double(), torch.from_numpy(want))     # representable
        for pdt in (torch.float32, torch_dtype(bits)):
            out = kernels.unpermute_rows(rows.to(DEV), _i32(imap), torch.from_numpy(probs).to(pdt).to(DEV), T)
            assert torch.equal(out.cpu(), ref.rounded(want, bits)), (T, k, E, pdt)
        # no probabilities = 1; a token whose every entry is -1 gets zeros
        imap2 = imap.copy()
        imap2[:, 0] = -1
        want, _ = ref.unpermute64(as64(rows), imap2, None)
        out = kernels.unpermute_rows(rows.to(DEV), _i32(imap2), None, T)
        assert torch.equal(out.cpu(), ref.rounded(want, bits)) and not bool(out[0].any()), (T, k, E)


@pytest.mark.parametrize("bits", ref.BITS)
def test_unpermute_on_random_data_stays_within_the_fp32_bound(bits):
    """|got - ref64| <= 1 ulp_T(ref64) + n_maps * 2^-23 * sum_m |p * x|: fp32 products and sums (each within 2^-24
    relative of a running value bounded by the sum of magnitudes), then one rounding to T"""
    from scalellm_amd import kernels
    rng = np.random.default_rng(4)
    dt = torch_dtype(bits)
    for form, T, k, E in (("index", 63, 3, 8), ("index", 257, 8, 256), ("mask", 65, 4, 64), ("mask", 16, 8, 256),
                          ("index", 2, 1, 4), ("mask", 64, 3, 7)):
        dim = ROW_DIMS[bits][-1]
        ids = ref.distinct_ids(rng, T, k, E)
        rows = ref.rounded(rng.standard_normal((T * k, dim)) * 3, bits)
        if form == "index":
            rmap, _ = ref.index_map(ids, E)
            probs = ref.rounded(rng.random((T, k)) + 0.01, "f32")
        else:
            rmap, _ = ref.mask_map(ref.ids_to_mask(ids, E))
            probs = ref.rounded(rng.random((T, E)) + 0.01, bits)                    # probs of the rows' dtype
        want, mag = ref.unpermute64(as64(rows), rmap, probs.double().numpy())
        out = kernels.unpermute_rows(rows.to(DEV), _i32(rmap), probs.to(DEV), T)
        err = np.abs(as64(out) - want)
        bound = ref.ulp(want, bits) + rmap.shape[0] * 2.0 ** -23 * mag
        worst = float((err / bound).max())
        print(f"[unpermute {bits} {form} T={T} k={k} E={E} dim={dim}] worst err / bound = {worst:.3f}")
        assert worst <= 1.0, (form, T, k, E, worst)
        assert torch.equal(kernels.unpermute_rows(rows.to(DEV), _i32(rmap), probs.to(DEV), T), out)   # repeats


# ---- graph replay ---------------------------------------------------------------------------------------------------------
def test_one_captured_graph_replays_over_three_routings():
    from scalellm_amd import kernels
    T, k, E, dim = 5, 2, 8, 64
    rng = np.random.default_rng(5)
    routings = [ref.distinct_ids(rng, T, k, E), ref.distinct_ids(rng, T, k, E), np.full((T, k), 3, dtype=np.int32)]
    routings[2][:, 1] = 9                                               # one expert takes all; slot 1 is foreign
    x = ref.rounded(rng.standard_normal((T, dim)), "bf16").to(DEV)
    probs = torch.full((T, k), 0.5, device=DEV)
    ids_s = _i32(routings[0])
    rmap_s = torch.empty(k, T, dtype=torch.int32, device=DEV)
    counts_s = torch.empty(E, dtype=torch.int32, device=DEV)
    perm_s = torch.zeros(T * k, dim, dtype=torch.bfloat16, device=DEV)
    out_s = torch.empty(T, dim, dtype=torch.bfloat16, device=DEV)

    def run():
        kernels.permute_with_index_map(x, ids_s, E, out=perm_s, row_id_map=rmap_s, tokens_per_expert=counts_s)
        kernels.unpermute_with_index_map(perm_s, rmap_s, probs, out=out_s)

    run()                                                              # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for ids in routings:
        ids_s.copy_(_i32(ids))
        perm_s.zero_()
        graph.replay()
        want_map, want_counts = ref.index_map(ids, E)
        assert np.array_equal(rmap_s.cpu().numpy(), want_map)
        assert np.array_equal(counts_s.cpu().numpy(), want_counts)
        want_perm = ref.permute_rows(x.cpu().view(torch.int16).numpy(), want_map, np.zeros((T * k, dim), np.int16))
        assert np.array_equal(perm_s.cpu().view(torch.int16).numpy(), want_perm)
        want, _ = ref.unpermute64(as64(perm_s), want_map, np.full((T, k), 0.5))
        assert torch.equal(out_s.cpu(), ref.rounded(want, "bf16"))
    torch.cuda.synchronize()


# ---- the C++ shim -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", ref.BITS)
def test_shim_functions_equal_the_ctypes_path(bits):
    from scalellm_amd import kernels
    from scalellm_amd.cpp_host import load_shim
    shim = load_shim()
    rng = np.random.default_rng(6)
    T, k, E, dim = 65, 3, 8, ROW_DIMS[bits][2]
    it = ref.int_dtype(bits)
    x = ref.rounded(rng.standard_normal((T, dim)), bits).to(DEV)
    ids = _i32(ref.distinct_ids(rng, T, k, E))
    p1, m1 = kernels.permute_with_index_map(x, ids)
    p2, m2 = shim.moe_permute_with_index_map(x, ids)
    assert m2.shape == (k * T,) and torch.equal(m1.view(-1), m2) and torch.equal(p1.view(it), p2.view(it))
    for probs in (torch.rand(T, k, device=DEV), torch.rand(T, k, device=DEV).to(x.dtype)):
        o1 = kernels.unpermute_with_index_map(p1, m1, probs)
        o2 = shim.moe_unpermute_with_index_map(p2, m2, probs)
        assert torch.equal(o1.view(it), o2.view(it)) and bool((o1 != 0).any())
    mask = torch.from_numpy(ref.ids_to_mask(ids.cpu().numpy(), E)).to(DEV)
    p1, m1 = kernels.permute_with_mask_map(x, mask, k)
    p2, m2 = shim.moe_permute_with_mask_map(x, mask, k)
    assert m2.shape == (E, T) and torch.equal(m1, m2) and torch.equal(p1.view(it), p2.view(it))
    probs = (torch.rand(T, E, device=DEV) * mask).to(x.dtype)
    o1 = kernels.unpermute_with_mask_map(p1, m1, probs)
    o2 = shim.moe_unpermute_with_mask_map(p2, m2, probs)
    assert torch.equal(o1.view(it), o2.view(it)) and bool((o1 != 0).any())
