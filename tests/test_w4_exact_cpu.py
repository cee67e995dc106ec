"""The recipe behind tests/test_w4_exact_gpu.py, checked without a GPU.

On inputs whose every product and partial sum is representable in fp32 (small-integer activations, power-of-two
scales, a bias that is a multiple of the smallest scale) an int4 GEMM does not depend on the order of summation, on
split-K or stream-K pieces, or on the dequant form: every kernel owes RNE_T(exact sum + bias) in every element.
Here, for every case of the GPU grid (tests/w4_exact_cases.py):
  * the exactness budget and the activation density hold (asserted where the inputs are made),
  * both dequant forms of csrc/w4_common.h, emulated in numpy fp32 with groups, k and partial sums in shuffled order,
    reproduce the float64 truth bit for bit,
  * on a subset the project's oracle (oracle.gemm_f32 over oracle.*_dequant) equals the truth exactly,
  * the plan query answers the kernel each case is meant for (a host-side query: the same assertion the GPU test
    makes, seen before any GPU time is spent),
and the bit comparison catches the localized faults that the mean metric of test_w4_gpu.py lets through.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import helpers
from tests import w4_exact_cases as cases

TDT = {"bf16": torch.bfloat16, "f16": torch.float16}


def _planes(q):
    """per packed row: integer weight, group id; per group: zero and fp32 scale.  An 8-bit layer is its two int4
    planes over 2K rows (csrc/w8_planes.hip): the high plane with 16 s, then the low plane with s."""
    K, gs = q["K"], q["group_size"]
    gi = q["g_idx"] if q["g_idx"] is not None else np.arange(K) // gs
    w, z, s = q["q"], q["z_eff"], q["scales"]
    if q.get("bits") != 8:
        return w, gi, z, s, 1
    G = z.shape[0]
    return (np.concatenate([w >> 4, w & 15]), np.concatenate([gi, gi + G]), np.concatenate([z >> 4, z & 15]),
            np.concatenate([16.0 * s, s]).astype(np.float32), 2)


def _round(acc, b, bits):
    if b is not None:
        acc = acc + b[None, :].astype(np.float32)      # fp32, then ONE rounding to T (pack2 / the reduce kernel)
    assert acc.dtype == np.float32
    return helpers._t_bits(acc, bits)


def _post_scaled(q, a, b, bits, rng):
    """s * (sum_k x_k (magic + q_k) - (magic + z) sum_k x_k) per group, all in fp32; groups, the k inside a group
    and the pieces a K slice cuts a group into in shuffled order"""
    w, gi, z, s, planes = _planes(q)
    a32 = np.concatenate([a] * planes, axis=1).astype(np.float32)
    magic = np.float32(helpers.EXACT_MAGIC[bits])
    acc = np.zeros((a.shape[0], q["N"]), np.float32)
    for g in rng.permutation(np.unique(gi)):
        ks = rng.permutation(np.flatnonzero(gi == g))
        s1 = np.zeros_like(acc)
        x = np.zeros(a.shape[0], np.float32)
        for part in np.array_split(ks, int(rng.integers(1, 4))):
            s1 += a32[:, part] @ (magic + w[part].astype(np.float32))
            x += a32[:, part].sum(axis=1, dtype=np.float32)
        acc += s[g][None, :] * (s1 - (magic + z[g].astype(np.float32))[None, :] * x[:, None])
    return _round(acc, b, bits)


def _pre_scaled(q, a, b, bits, rng):
    """T((q - z) s) times x, k in shuffled order, 2..7 partial sums (split-K slabs, stream-K pieces) added in fp32"""
    w, gi, z, s, planes = _planes(q)
    a32 = np.concatenate([a] * planes, axis=1).astype(np.float32)
    wt = (w - z[gi]).astype(np.float32) * s[gi]
    assert np.array_equal(helpers._from_t_bits(helpers._t_bits(wt, bits), bits), wt)   # <= 5 significant bits
    acc = np.zeros((a.shape[0], q["N"]), np.float32)
    for part in np.array_split(rng.permutation(wt.shape[0]), int(rng.integers(2, 8))):
        acc += a32[:, part] @ wt[part]
    return _round(acc, b, bits)


def _want_bits(truth, bits):
    return torch.from_numpy(truth).to(TDT[bits]).view(torch.int16).numpy().view(np.uint16)


def _check_recipe(q, a, b, truth, bits, what, seed=0):
    rng = np.random.default_rng(seed)
    want = _want_bits(truth, bits)
    for form in (_post_scaled, _pre_scaled):
        got = form(q, a, b, bits, rng)
        assert np.array_equal(got, want), (what, form.__name__, int((got != want).sum()))


def _all_groups():
    return cases.dense_groups() + cases.STRIDED + cases.SILU


@pytest.mark.parametrize("bits", cases.BITS)
def test_recipe_dense_cases(bits):
    """every (shape, bias) of the dense, strided and SiLU groups, once (the groups share shapes across knobs)"""
    seen = set()
    for group in _all_groups():
        for case in cases.cases_of(group, bits):
            key = case[:7]
            if key in seen:
                continue
            seen.add(key)
            q, a, b, truth, share = cases.inputs(bits, case)
            _check_recipe(q, a, b, truth, bits, (group.name, key), seed=len(seen))
            # the rounding and its ties are exercised: bf16 from K = 512 on, f16 wherever the (big) bias is on
            cases.assert_share(bits, case.K, case.bias, share, (group.name, key))
    assert len(seen) > 60
    for group in cases.dense_groups():    # f16 outputs need rounding under the big bias only: every kernel has such a case
        assert any(case.bias for case in cases.cases_of(group, bits)), group.name
    for kernel in {g.kernel for g in cases.SILU if g.kernel}:       # ... and so does every kernel's SiLU epilogue
        assert any(case.bias for g in cases.SILU if g.kernel == kernel for case in cases.cases_of(g, bits)), kernel


@pytest.mark.parametrize("bits", cases.BITS)
@pytest.mark.parametrize("n", range(len(cases.XL_SK)))
def test_recipe_stream_k_cases(bits, n):
    case = cases.XL_SK[n]
    q, a, b, truth, share = cases.inputs(bits, case)
    # the emulation does not depend on M: a band of rows at both ends keeps this quick
    rows = np.r_[0:48, case.M - 48:case.M]
    _check_recipe(q, a[rows], b, truth[rows], bits, case[:7], seed=n)
    cases.assert_share(bits, case.K, case.bias, share, case[:7])


@pytest.mark.parametrize("bits", cases.BITS)
def test_recipe_deferred_gemv_and_shards(bits):
    M, N, K, _ = cases.GEMV_DEFERRED[bits]
    q, a, b, truth, _ = cases.inputs(bits, cases._c(M, N, K, 128, "awq"))
    _check_recipe(q, a, b, truth, bits, "deferred GEMV")
    for world, M, N, K, gs in cases.SHARDS:
        q, a, b, truth, _ = cases.inputs(bits, cases._c(M, N, K, gs, "gptq", act=True))
        parts = cases.shard_truths(q, a, world)
        assert np.array_equal(sum(parts), truth)          # the ranks' partial truths are the layer's
        ks = K // world
        for r in range(world):
            shard = cases.shard_case(q, r, world)
            helpers.assert_exact_budget(a[:, r * ks:(r + 1) * ks], shard)
            _check_recipe(shard, a[:, r * ks:(r + 1) * ks], None, parts[r], bits, ("shard", world, r))
            cases.assert_share(bits, ks, False, cases.share_of(parts[r], bits), ("shard", world, r, ks))


@pytest.mark.parametrize("bits", cases.BITS)
def test_recipe_8bit_cases(bits):
    for n in range(len(cases.W8_CASES[bits])):
        for M in cases.W8_M:
            q, a, b, truth, share = cases.inputs8(bits, n, M)
            _check_recipe(q, a, b, truth, bits, ("w8", n, M), seed=M)
            cases.assert_share(bits, q["K"], b is not None, share, ("w8", n, M))


@pytest.mark.parametrize("bits", cases.BITS)
def test_recipe_moe_cases(bits):
    for n in range(len(cases.MOE)):
        experts, ids, a_tok, a_flat, row_scale = cases.moe_inputs(bits, n)
        k = ids.shape[1]
        for a, a_div in ((a_tok, k), (a_flat, 1)):
            truth = cases.moe_truth(experts, ids, a, a_div)
            flat = ids.reshape(-1)
            for e in np.unique(flat):
                f = np.flatnonzero(flat == e)
                _check_recipe(experts[e], a[f // a_div], None, truth[f], bits, ("moe", n, a_div, int(e)))
            cases.assert_share(bits, cases.MOE[n][2], False, cases.share_of(truth, bits), ("moe", n, a_div))


@pytest.mark.parametrize("bits", cases.BITS)
def test_oracle_agrees_with_the_truth_exactly(bits):
    """oracle.gemm_f32 over oracle.*_dequant (what every other int4 test is measured against) on the M <= 8 cases"""
    n = 0
    for group in (cases.GEMV, cases.KS1, cases.SMALL[0]):
        for case in cases.cases_of(group, bits):
            if case.M > 8:
                continue
            q, a, b, truth, _ = cases.inputs(bits, case)
            if case.fmt == "awq":
                w = oracle.awq_dequant(q["qweight"], q["qzeros"], q["scales"], q["group_size"])
            else:
                w = oracle.gptq_dequant(q["qweight"], q["qzeros"], q["scales"], q["group_size"], q["g_idx"])
            got = oracle.gemm_f32(a, w).astype(np.float64)
            if b is not None:
                got = got + b[None, :].astype(np.float64)
            assert np.array_equal(got, truth), (group.name, case[:7])
            n += 1
    for i in range(len(cases.W8_CASES[bits])):
        q, a, b, truth, _ = cases.inputs8(bits, i, 1)
        if q["fmt"] == "awq":
            w = oracle.awq_dequant(q["qweight"], q["qzeros"], q["scales"], q["group_size"], bits=8)
        else:
            w = oracle.gptq_dequant(q["qweight"], q["qzeros"], q["scales"], q["group_size"], q["g_idx"], bits=8)
        got = oracle.gemm_f32(a, w).astype(np.float64) + (0 if b is None else b[None, :].astype(np.float64))
        assert np.array_equal(got, truth), ("w8", i)
        n += 1
    assert n >= 10


# ---- the plan of every case, asked on the host ------------------------------------------------------------------
def _plan(bits, M, N, K, gs, perm, bias, flags=0, lda=None, ldc=None):
    from scalellm_amd import _lib
    g = _lib.W4GemmArgs()
    g.M, g.K, g.N, g.lda, g.ldc = M, K, N, lda or K, ldc or N
    g.group_size = K if gs in (-1, 0) else gs
    g.dtype = _lib.SLM_BF16 if bits == "bf16" else _lib.SLM_F16
    g.flags = flags
    g.perm = 1 if perm else None       # (never dereferenced: the plan only asks whether there is one)
    g.bias = 1 if bias else None
    info = _lib.W4PlanInfo()
    assert _lib.lib().slm_w4a16_gemm_plan(C.byref(g), C.byref(info)) == 0
    return info, int(_lib.lib().slm_w4a16_gemm_deferred_splits(C.byref(g)))


@pytest.mark.parametrize("bits", cases.BITS)
def test_every_case_plans_the_kernel_it_is_meant_for(bits):
    from scalellm_amd import _lib, kernels
    for group in _all_groups():
        silu = group.name.startswith("silu")
        for case in cases.cases_of(group, bits):
            with kernels.tuning(**{**group.knobs, **case.knobs}):
                for flags in ((0, _lib.SLM_W4_SILU_MUL) if silu else (0,)):
                    plan, _ = _plan(bits, case.M, case.N, case.K, case.gs, case.act, case.bias, flags,
                                    ldc=case.N // 2 if flags else None)
                    cases.check_plan(group, case, plan)
    for _, knobs, kernel in cases.XL_SK_FORMS:
        with kernels.tuning(**knobs):
            for case in cases.XL_SK:
                cases.check_xl_plan(case, kernel, _plan(bits, case.M, case.N, case.K, case.gs, False, case.bias)[0])
    M, N, K, knobs = cases.GEMV_DEFERRED[bits]
    with kernels.tuning(**knobs):
        plan, deferred = _plan(bits, M, N, K, 128, False, False, _lib.SLM_W4_DEFER_REDUCE)
    assert plan.kernel_name == "GEMV" and 2 <= deferred <= 4
    for world, M, N, K, gs in cases.SHARDS:      # an uneven shard: padded rows in blocks of 32, one scale row per block
        q = cases.inputs(bits, cases._c(M, N, K, gs, "gptq", act=True))[0]
        for r in range(world):
            g_idx = torch.from_numpy(cases.shard_case(q, r, world)["g_idx"]).to(torch.int64)
            perm_p, _ = kernels.plan_uneven_groups(g_idx, torch.argsort(g_idx, stable=True), K // gs)
            cases.check_shard_plan(perm_p.numel(), _plan(bits, M, N, perm_p.numel(), 32, True, False, lda=K)[0],
                                   (world, r, M, N, K, gs))
    seen = set()
    for n, (N, K, gs, *_rest) in enumerate(cases.W8_CASES[bits]):   # two planes: 2K packed rows, always gathered
        for M in cases.W8_M:
            gp = int(_lib.lib().slm_w8_packed_group_size(K, gs))
            plan = _plan(bits, M, N, 2 * K, gp, True, M % 2 == 1)[0]
            assert gp > 0
            cases.check_w8_plan(M, 2 * K, gp, plan, (n, M))
            seen.add((plan.kernel_name, plan.row_tiles))
    assert seen >= {("GEMV", 0), ("KS", 1), ("KS", 2), ("GENERAL", 2)}, seen


# ---- what the bit comparison sees and the mean metric does not --------------------------------------------------
GEMM_TOL = {"f16": 1e-3, "bf16": 8e-3}   # tests/test_w4_gpu.py


def _mean_metric(c, ref):
    return float(np.abs(c - ref).mean() / np.abs(ref).mean())


@pytest.mark.parametrize("bits", cases.BITS)
def test_bit_comparison_catches_the_faults_the_mean_metric_misses(bits, capsys):
    # a whole row is 1 / M of the mean: bf16's bound lets one through at the M = 300 of the forced-kernel grids,
    # f16's eight times tighter bound at the row counts of the stream-K grid (M = 2048...4000)
    M, N, K, gs = {"bf16": 300, "f16": 3000}[bits], 160, 1024, 128
    T = TDT[bits]
    q = helpers.make_exact_quant_case(77, K, N, gs, "gptq", bits)
    a = helpers.exact_activations(77, M, K, helpers.EXACT_XMAX[bits])
    b = helpers.exact_bias(77, N, q)
    helpers.assert_exact_budget(a, q, b)
    truth, share = helpers.exact_truth(a, q, b)
    good = torch.from_numpy(truth).to(T)
    helpers.assert_bits_equal(good, truth, T, "clean")
    w = helpers._exact_weight(q)

    def fault(name):
        c = good.clone()
        if name == "one element off by one ulp":
            v = c.view(torch.int16)
            v[123, 45] += 1
        elif name == "last row zeroed":
            c[M - 1] = 0
        elif name == "last row replaced by row 0":
            c[M - 1] = c[0]
        elif name == "one 32x32 tile without one 64-deep chunk":
            part = truth[256:288, 96:128] - a[256:288, 512:576].astype(np.float64) @ w[512:576, 96:128]
            c[256:288, 96:128] = torch.from_numpy(part).to(T)
        elif name == "one column without bias":
            col = int(np.argmax(np.abs(b)))
            c[:, col] = torch.from_numpy(truth[:, col] - float(b[col])).to(T)
        elif name == "two rows swapped":
            c[[7, 200]] = c[[200, 7]]
        elif name == "one column with its neighbour group's scale":
            g, col = [int(i[0]) for i in np.nonzero(q["scales"][:-1] != q["scales"][1:])]
            ks = slice(g * gs, (g + 1) * gs)
            wrong = truth[:, col] + a[:, ks].astype(np.float64) @ (
                w[ks, col] * (float(q["scales"][g + 1, col]) / float(q["scales"][g, col]) - 1.0))
            c[:, col] = torch.from_numpy(wrong).to(T)
        return c

    names = ["one element off by one ulp", "last row zeroed", "last row replaced by row 0",
             "one 32x32 tile without one 64-deep chunk", "one column without bias", "two rows swapped",
             "one column with its neighbour group's scale"]
    clean = _mean_metric(good.float().numpy().astype(np.float64), truth)
    print(f"\n[{bits}] share needing rounding {share:.3f}; clean mean metric {clean:.2e} (bound {GEMM_TOL[bits]:.0e})")
    for i, name in enumerate(names):
        c = fault(name)
        assert not torch.equal(c.view(torch.int16), good.view(torch.int16)), name    # the fault is a fault
        with pytest.raises(AssertionError, match="differ from RNE") as err:
            helpers.assert_bits_equal(c, truth, T, name)
        metric = _mean_metric(c.float().numpy().astype(np.float64), truth)
        print(f"[{bits}] {name}: mean metric {metric:.2e}; {str(err.value)[:150]}")
        if i < 5:   # the reason for this file: the old metric passes these
            assert metric < GEMM_TOL[bits], (name, metric)
    # the message tells a tile from a row: the bounding box of the tile fault is the tile
    with pytest.raises(AssertionError, match=r"rows \[256, 287\].*columns \[96, 127\]"):
        helpers.assert_bits_equal(fault(names[3]), truth, T, names[3])
