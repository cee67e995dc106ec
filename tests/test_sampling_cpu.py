"""CPU tests of the sampling boundary (include/slm_hip.h section 8): the numpy oracle's Philox stream
against rocRAND, the oracle against hand-worked cases of every step of the contract, the ctypes
mirror of slm_sampling_args, and argument validation before any launch."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from scalellm_amd import _lib
from scalellm_amd._lib import SamplingArgs

from . import sampling_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
PHILOX_H = os.path.join(ROCM, "include", "rocrand", "rocrand_philox4x32_10.h")

F32 = np.float32
NINF = F32(-np.inf)


@pytest.mark.skipif(not os.path.exists(PHILOX_H) or shutil.which("g++") is None,
                    reason="rocRAND header or host compiler absent")
def test_philox_oracle_matches_rocrand(tmp_path):
    """draw(seed, position, i) == philox4x32_10_engine(seed, position | stream << 32, i).next(): the rocRAND
    engine built as a plain host program (the header is __host__ __device__)."""
    src = tmp_path / "philox.cpp"
    src.write_text(
        "#include <rocrand/rocrand_philox4x32_10.h>\n#include <cstdio>\n#include <cstdlib>\n"
        "int main(int argc, char** argv) {\n"
        "  for (int a = 1; a + 2 < argc; a += 3) {\n"
        "    rocrand_device::philox4x32_10_engine e(strtoull(argv[a], 0, 10), strtoull(argv[a + 1], 0, 10),\n"
        "                                           strtoull(argv[a + 2], 0, 10));\n"
        "    printf(\"%u\\n\", e.next());\n  }\n  return 0;\n}\n")
    exe = tmp_path / "philox"
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__=1", f"-I{ROCM}/include", str(src),
                           "-o", str(exe)])
    rng = np.random.default_rng(7)
    seeds = [0, 1, 0xDEADBEEF, (1 << 64) - 1, 0x0123456789ABCDEF] + [int(s) for s in rng.integers(0, 2**63, 5)]
    cases = []
    for s in seeds:
        for pos in (0, 1, 4095, 131071, 2**31 - 1):
            for i in (0, 1, 2, 3, 4, 7, 1023, 50256, 128255) + tuple(int(v) for v in rng.integers(0, 1 << 22, 4)):
                cases.append((s, pos, i))
    args = [str(v) for c in cases for v in c]
    got = []
    for k in range(0, len(args), 3 * 400):
        got += [int(v) for v in subprocess.check_output([str(exe), *args[k:k + 3 * 400]], text=True).split()]
    assert len(got) == len(cases)
    for (s, pos, i), want in zip(cases, got):
        assert int(ref.philox_words(s, pos, [i])[0]) == want, (s, pos, i)
    # stream 1 (room for a rejection sampler) is a different subsequence
    w = subprocess.check_output([str(exe), "5", str(3 | (1 << 32)), "9"], text=True).split()
    assert int(ref.philox_words(5, 3, [9], stream=1)[0]) == int(w[0])


def test_exp_draws_stay_positive_and_monotone():
    m = np.array([0, 1, (1 << 23) - 1, 1 << 23, (1 << 24) - 2, (1 << 24) - 1], dtype=np.uint32)
    E = ref.exp_draws(m << np.uint32(8))
    assert np.all(E > 0) and np.all(np.isfinite(E))
    assert np.all(np.diff(E.astype(np.float64)) < 0)   # larger u, smaller E
    np.testing.assert_allclose(E, -np.log((m.astype(np.float64) + 0.5) / 2**24), rtol=1e-6)


def test_oracle_penalties_exact_float32_steps():
    x = np.array([1.5, -2.0, 0.25, 3.0, -0.5], F32)
    ids, counts = np.array([3, 1, 0, 4]), np.array([2, 1, 0, 3])
    out, _ = ref.process_row(x, freq=0.3, pres=0.5, rep=1.25, ids=ids, counts=counts, n_ids=3)
    # id 3: (3 - F32(2 * 0.3)) - 0.5, then / 1.25
    a = F32(F32(F32(3.0) - F32(F32(2) * F32(0.3))) - F32(0.5))
    assert out[3] == F32(a / F32(1.25))
    b = F32(F32(F32(-2.0) - F32(F32(1) * F32(0.3))) - F32(0.5))
    assert out[1] == F32(b * F32(1.25))                   # negative: multiplied
    assert out[0] == F32(F32(1.5) / F32(1.25))            # count 0: repetition only
    assert out[4] == F32(-0.5) and out[2] == F32(0.25)    # beyond lens (padding): untouched
    # temperature: the fp32 reciprocal, t == 0 -> 1
    t, _ = ref.process_row(x, temp=0.7)
    np.testing.assert_array_equal(t, x * F32(F32(1) / F32(0.7)))
    t0, _ = ref.process_row(x, temp=0.0)
    np.testing.assert_array_equal(t0, x)


def test_oracle_top_k_top_p_and_tie_rules():
    x = np.array([1.0, 3.0, 3.0, 2.0, 3.0, 0.0], F32)
    out, _ = ref.process_row(x, top_k=2)                  # three 3.0s: the two lowest ids win
    np.testing.assert_array_equal(out, [NINF, 3, 3, NINF, NINF, NINF])
    out, _ = ref.process_row(x, top_k=1)
    np.testing.assert_array_equal(out, [NINF, 3, NINF, NINF, NINF, NINF])
    out, _ = ref.process_row(x, top_k=0)                  # off
    np.testing.assert_array_equal(out, x)
    out, _ = ref.process_row(x, top_k=6)                  # k >= vocab: off
    np.testing.assert_array_equal(out, x)
    out, _ = ref.process_row(x, top_p=0.0)                # rank 0 only
    np.testing.assert_array_equal(out, [NINF, 3, NINF, NINF, NINF, NINF])
    # probs of [log 4, log 2, log 1, log 1] = [.5, .25, .125, .125]; exclusive sums 0, .5, .75, .875
    y = np.log(np.array([4, 2, 1, 1], np.float64)).astype(F32)
    out, excl = ref.process_row(y, top_p=0.5)             # keep ranks with sum before <= 0.5
    np.testing.assert_array_equal(np.isfinite(out), [True, True, False, False])
    out, _ = ref.process_row(y, top_p=0.8)
    np.testing.assert_array_equal(np.isfinite(out), [True, True, True, False])
    out, _ = ref.process_row(y, top_k=3, top_p=0.6)       # top-p over the top-k survivors: .571, .286
    np.testing.assert_array_equal(np.isfinite(out), [True, True, False, False])
    out, _ = ref.process_row(y, top_p=1.0)
    np.testing.assert_array_equal(out, y)
    # -0 == +0: a tie, the lower id first
    z = np.array([-0.0, 0.0, -1.0], F32)
    out, _ = ref.process_row(z, top_k=1)
    assert np.isfinite(out[0]) and not np.isfinite(out[1])


def test_oracle_sampling_greedy_race_and_logprobs():
    x = np.array([0.5, 2.0, 2.0, -1.0], F32)
    assert ref.sample_row(x, False, 1, 0) == 1            # greedy: argmax, lowest id on ties
    # equal logits: the race is argmax of the uniform stream (ties: lowest id)
    e = np.zeros(1024, F32)
    for seed, pos in ((1, 0), (12345, 77), ((1 << 64) - 1, 9)):
        u = ref.uniform24(ref.philox_words(seed, pos, np.arange(1024)))
        assert ref.sample_row(e, True, seed, pos) == int(np.argmax(u))
    # a filtered token never wins
    f = np.array([NINF, 0.0, NINF, 0.0], F32)
    for seed in range(50):
        assert ref.sample_row(f, True, seed, 3) in (1, 3)
    lp, top_v, top_i = ref.logprobs_row(f, 1, 3)
    assert lp == pytest.approx(np.log(0.5))
    np.testing.assert_array_equal(top_i, [1, 3, 0])       # -inf ties: lowest id
    assert top_v[2] == -np.inf


def _args(**kw):
    a = SamplingArgs()
    a.logits, a.logits_stride, a.dtype, a.n_rows, a.vocab = 4096, 1024, 1, 2, 1024
    a.next_tokens = 8192
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_sampling_argument_validation_precedes_any_launch():
    L = _lib.lib()
    S, P = L.slm_sample, L.slm_logits_process
    assert S(None, None) == -1
    assert S(C.byref(_args(logits=None)), None) == -1               # NULL logits
    assert S(C.byref(_args(next_tokens=None)), None) == -1          # slm_sample needs the token buffer
    assert S(C.byref(_args(n_top=21, top_logprobs=4096, top_tokens=4096)), None) == -1   # n_top > 20
    assert S(C.byref(_args(n_top=2)), None) == -1                   # top-n without its buffers
    assert S(C.byref(_args(vocab=8, logits_stride=8, n_top=9, top_logprobs=4096, top_tokens=4096)), None) == -1
    assert S(C.byref(_args(dtype=3)), None) == -2                   # bad dtype
    assert S(C.byref(_args(vocab=(1 << 22) + 1, logits_stride=(1 << 22) + 1)), None) == -2
    assert S(C.byref(_args(logits_stride=1000)), None) == -1        # stride < vocab
    assert S(C.byref(_args(n_rows=-1)), None) == -1
    assert S(C.byref(_args(n_rows=0)), None) == 0                   # empty batch: no-op
    assert S(C.byref(_args(n_rows=0, logits=None)), None) == 0
    assert S(C.byref(_args(repetition_penalties=4096, max_unique=4)), None) == -1       # no ids / lens
    assert S(C.byref(_args(frequency_penalties=4096, unique_ids=4096, unique_lens=4096, max_unique=4)),
             None) == -1                                                                # no counts
    assert S(C.byref(_args(repetition_penalties=4096, unique_ids=4096, unique_lens=4096, max_unique=4,
                           vocab=(1 << 19) + 1, logits_stride=(1 << 19) + 1)), None) == -2
    pen = dict(repetition_penalties=4096, unique_ids=4096, unique_lens=4096, max_unique=64)
    assert L.slm_sample_workspace_bytes(C.byref(_args(**pen))) == 2 * 64 * 4   # [n_rows, max_unique] fp32
    assert L.slm_sample_workspace_bytes(C.byref(_args())) == 0
    assert S(C.byref(_args(**pen)), None) == -3                     # workspace missing
    assert P(C.byref(_args()), None) == -1                          # processing needs `processed`
    assert P(C.byref(_args(processed=4096, processed_stride=1000)), None) == -1
    # in place, no processing step given: nothing to do, nothing launched
    assert P(C.byref(_args(processed=4096, processed_stride=1024)), None) == 0


def test_sampling_args_match_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(slm_sampling_args));']
    for fname, _ in SamplingArgs._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(slm_sampling_args, {fname}));')
    lines += ['  printf("SLM_F32 %d\\n", (int)SLM_F32);', '  printf("MAX_TOP %d\\n", SLM_SAMPLE_MAX_TOP);',
              '  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out.pop("size")) == C.sizeof(SamplingArgs)
    assert int(out.pop("SLM_F32")) == _lib.SLM_F32
    assert int(out.pop("MAX_TOP")) == _lib.SLM_SAMPLE_MAX_TOP
    for fname, _ in SamplingArgs._fields_:
        assert int(out[fname]) == getattr(SamplingArgs, fname).offset, fname


def test_sampling_parameters_on_the_host():
    """SamplingParameter draws a seed when none is given; the python API exists without a GPU."""
    from scalellm_amd.sampling import LogitsProcessor, SampleOutput, Sampler, SamplingParameter, sample_logits  # noqa
    a, b = SamplingParameter(), SamplingParameter()
    assert 0 <= a.seed < 2**64 and a.seed != b.seed
    assert SamplingParameter(seed=-1).seed == 2**64 - 1
    assert SamplingParameter().temperature == pytest.approx(0.7)   # the reference's default


def test_refresh_from_a_compact_batch_writes_neutral_values():
    """copy_() into the max-batch tensors a captured step reads: a field the source leaves None (neutral
    for all its rows) must overwrite what the previous batch left there."""
    import torch
    from scalellm_amd.sampling import SamplingParameter, SamplingParameters
    big = SamplingParameters.create([SamplingParameter(do_sample=True, top_k=5, top_p=0.5, repetition_penalty=1.3,
                                                       frequency_penalty=0.2, presence_penalty=0.1, seed=9)] * 3,
                                    [[1, 2], [3, 4], [5, 6]], device="cpu", compact=False, max_unique=4)
    small = SamplingParameters.create([SamplingParameter(temperature=1.0, seed=7)] * 2, device="cpu")
    assert small.do_sample is None and small.top_k is None and small.unique_token_ids is None
    big.copy_(small)
    assert big.do_sample[:2].tolist() == [False, False] and big.do_sample[2].item()
    assert big.top_k[:2].tolist() == [-1, -1] and big.top_p[:2].tolist() == [1.0, 1.0]
    assert big.repetition_penalties[:2].tolist() == [1.0, 1.0]
    assert big.frequency_penalties[:2].tolist() == [0.0, 0.0] and big.presence_penalties[:2].tolist() == [0.0, 0.0]
    assert big.unique_token_ids_lens[:2].tolist() == [0, 0] and int(big.unique_token_ids[:2].abs().sum()) == 0
    assert big.temperatures[:2].tolist() == [1.0, 1.0] and big.seeds[:2].tolist() == [7, 7]
    assert big.unique_token_ids_lens[2].item() == 2            # rows beyond the new batch are left alone
    with pytest.raises(Exception):                              # a batch larger than the buffers
        big.copy_(SamplingParameters.create([SamplingParameter()] * 4, device="cpu"))
    assert torch.equal(big.top_k[:2], torch.tensor([-1, -1]))
