"""CPU tests of the rejection-sampling boundary (include/slm_hip.h section 9): the header and the library
agree, the ctypes mirror of slm_rejection_args matches the C layout, argument validation precedes any
launch, build_accepted_mask reproduces the reference's Mask case, and the restatement's stream-1 and
stream-2 draws are rocRAND's philox4x32_10_engine(seed, position | stream << 32, i)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from scalellm_amd import _lib
from scalellm_amd._lib import RejectionArgs

from . import rejection_ref as rref
from . import sampling_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slm_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "rejection_sampler_cases.npz")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
PHILOX_H = os.path.join(ROCM, "include", "rocrand", "rocrand_philox4x32_10.h")


def test_header_declares_the_rejection_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = set(re.findall(r"SLM_API\s+[\w\s\*]+?\b(slm_\w+)\s*\(", src))
    assert {"slm_rejection_sample", "slm_rejection_sample_workspace_bytes"} <= syms
    L = _lib.lib()  # binds both: an AttributeError here is a header / library mismatch
    assert L.slm_rejection_sample and L.slm_rejection_sample_workspace_bytes


def test_rejection_args_match_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slm_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(slm_rejection_args));']
    for fname, _ in RejectionArgs._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(slm_rejection_args, {fname}));')
    lines += ['  printf("MAX_K %d\\n", SLM_REJECTION_MAX_K);', '  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out.pop("size")) == C.sizeof(RejectionArgs)
    assert int(out.pop("MAX_K")) == _lib.SLM_REJECTION_MAX_K
    assert set(out) == {f for f, _ in RejectionArgs._fields_}
    for fname, _ in RejectionArgs._fields_:
        assert int(out[fname]) == getattr(RejectionArgs, fname).offset, fname


def _args(**kw):
    """A well-formed call on fake (never dereferenced) pointers: n = 2, k = 4, vocab 1024, bf16 logits."""
    a = RejectionArgs()
    base = dict(n_seqs=2, k=4, vocab=1024, dtype=_lib.SLM_BF16, draft_token_ids=4096, draft_probs=4096,
                draft_seq_stride=4 * 1024, draft_row_stride=1024, target=4096, target_seq_stride=5 * 1024,
                target_row_stride=1024, bonus_token_ids=4096, next_tokens=4096)
    base.update(kw)
    for name, v in base.items():
        setattr(a, name, v)
    return a


def test_rejection_argument_validation_precedes_any_launch():
    L = _lib.lib()
    R = L.slm_rejection_sample
    assert R(None, None) == -1
    assert R(C.byref(_args(n_seqs=-1)), None) == -1
    assert R(C.byref(_args(n_seqs=0)), None) == 0                       # empty batch: no-op
    assert R(C.byref(_args(n_seqs=0, target=None)), None) == 0
    for name in ("draft_token_ids", "target", "bonus_token_ids", "next_tokens"):
        assert R(C.byref(_args(**{name: None})), None) == -1, name     # required pointers
    assert R(C.byref(_args(k=0)), None) == -1
    assert R(C.byref(_args(k=17, target_seq_stride=18 * 1024, draft_seq_stride=17 * 1024)), None) == -1
    assert R(C.byref(_args(n_top=21, top_logprobs=4096, top_tokens=4096)), None) == -1
    assert R(C.byref(_args(n_top=2)), None) == -1                       # top-n without its buffers
    assert R(C.byref(_args(vocab=8, target_row_stride=8, target_seq_stride=40, draft_row_stride=8,
                           draft_seq_stride=32, n_top=9, top_logprobs=4096, top_tokens=4096)), None) == -1
    assert R(C.byref(_args(dtype=_lib.SLM_F32, target_is_probs=1, target_seq_stride=4 * 1024,
                           logprobs=4096)), None) == -1                 # logprobs need logits
    assert R(C.byref(_args(dtype=3)), None) == -2                       # bad dtype
    assert R(C.byref(_args(target_is_probs=1)), None) == -2             # probabilities are fp32
    big = (1 << 22) + 1
    assert R(C.byref(_args(vocab=big, target_row_stride=big, target_seq_stride=5 * big, draft_row_stride=big,
                           draft_seq_stride=4 * big)), None) == -2
    assert R(C.byref(_args(target_row_stride=1000)), None) == -1        # row stride < vocab
    assert R(C.byref(_args(draft_row_stride=1000)), None) == -1
    assert R(C.byref(_args(target_seq_stride=-1)), None) == -1
    assert R(C.byref(_args(draft_seq_stride=-1)), None) == -1
    # read-only inputs may interleave: a [k + 1, n, V] buffer viewed as [n, k + 1, V] passes validation
    assert R(C.byref(_args(target_seq_stride=1024, target_row_stride=2 * 1024, draft_seq_stride=1024,
                           draft_row_stride=2 * 1024)), None) == -3
    # a probability target has k rows; the draft stride is not checked without draft_probs
    assert R(C.byref(_args(dtype=_lib.SLM_F32, target_is_probs=1, target_seq_stride=4 * 1024)), None) == -3
    assert R(C.byref(_args(draft_probs=None, draft_seq_stride=0)), None) == -3
    need = L.slm_rejection_sample_workspace_bytes(C.byref(_args()))
    assert R(C.byref(_args()), None) == -3                              # workspace missing
    assert R(C.byref(_args(workspace=4096, workspace_bytes=need - 1)), None) == -3


def test_workspace_bytes_is_a_pure_function_of_sizes():
    L = _lib.lib()
    W = L.slm_rejection_sample_workspace_bytes
    assert W(None) == 0
    assert W(C.byref(_args(n_seqs=0))) == 0
    assert W(C.byref(_args(n_seqs=2, k=4))) == 256                     # 2 * 5 * 16 bytes, 256-aligned
    assert W(C.byref(_args(n_seqs=256, k=4, vocab=128256, target=None))) == 256 * 5 * 16
    assert W(C.byref(_args(n_seqs=3, k=16))) == 3 * 17 * 16 + 256 - (3 * 17 * 16) % 256


def test_build_accepted_mask_reproduces_the_reference_mask_case():
    from scalellm_amd.speculative import RejectionSampler
    g = np.load(GOLDEN)
    got = RejectionSampler.build_accepted_mask(torch.from_numpy(g["mask_accepted"]))
    np.testing.assert_array_equal(got.numpy(), g["mask_expected"])
    np.testing.assert_array_equal(rref.build_accepted_mask(g["mask_accepted"]), g["mask_expected"])


def test_restatement_reproduces_the_basic_case_decisions():
    """The given uniforms accept rows [1, 1, 0]; the recovered token of row 2 is one of the ids with p > q."""
    g = np.load(GOLDEN)
    r = rref.validate_seq(g["basic_draft_token_ids"][0], g["basic_draft_probs"][0], g["basic_target_probs"][0],
                          int(g["basic_bonus_token_ids"][0]), do_sample=True, uniform=g["basic_uniform"][0],
                          target_is_probs=True)
    np.testing.assert_array_equal(r["accepted"], g["basic_accepted"][0])
    exp = g["basic_expected_output"][0]
    assert list(r["tokens"][[0, 1, 3]]) == list(exp[[0, 1, 3]])
    p, q = g["basic_target_probs"][0, 2], g["basic_draft_probs"][0, 2]
    assert r["tokens"][2] in set(np.nonzero(p > q)[0]) == {2, 4}
    assert list(r["masked"]) == [1, 2, int(r["tokens"][2]), -1]


def _philox_py(key, ctr):
    """Philox4x32-10 in plain Python integers (independent of the numpy restatement)."""
    c = list(ctr)
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k1) & 0xFFFFFFFF,
             p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def _rocrand_formula(seed, position, stream, i):
    """philox4x32_10_engine(seed, subsequence = position | stream << 32, offset = i).next(): counter
    (lo32(i >> 2), hi32(i >> 2), lo32(subsequence), hi32(subsequence)), word i & 3."""
    sub = (position & 0xFFFFFFFF) | (stream << 32)
    q = i >> 2
    return _philox_py(seed, [q & 0xFFFFFFFF, q >> 32, sub & 0xFFFFFFFF, sub >> 32])[i & 3]


def test_stream_1_and_2_words_equal_the_rocrand_formula():
    # Random123's known answer for Philox4x32-10 (counter 0, key 0) anchors the plain-Python engine
    assert _philox_py(0, [0, 0, 0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    rng = np.random.default_rng(5)
    for seed in [0, 1, (1 << 64) - 1] + [int(s) for s in rng.integers(0, 2**63, 3)]:
        for pos in (0, 7, 2**31 - 1):
            ids = [0, 1, 2, 3, 4, 5, 50256, 128255]
            for stream in (1, 2):
                got = sref.philox_words(seed, pos, ids, stream=stream)
                want = [_rocrand_formula(seed, pos, stream, i) for i in ids]
                assert [int(x) for x in got] == want, (seed, pos, stream)
            # the acceptance draw: word 0 of stream 1 at position + j
            for j in (0, 3):
                x = _rocrand_formula(seed, (pos + j) & 0xFFFFFFFF, 1, 0)
                assert rref.acceptance_uniform(seed, pos, j) == np.float32(((x >> 8) + 0.5) * 2.0 ** -24)
            # streams 1 and 2 differ from stream 0 at the same seed and position
            assert list(sref.philox_words(seed, pos, ids, stream=0)) != list(sref.philox_words(seed, pos, ids, 2))


@pytest.mark.skipif(not os.path.exists(PHILOX_H) or shutil.which("g++") is None,
                    reason="rocRAND header or host compiler absent")
def test_stream_words_match_the_rocrand_engine(tmp_path):
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
    cases = [(s, p, st, i) for s in (0, 12345, (1 << 64) - 1) for p in (0, 99, 2**31 - 1) for st in (1, 2)
             for i in (0, 1, 3, 4, 1023, 128255)]
    args = [str(v) for s, p, st, i in cases for v in (s, p | (st << 32), i)]
    got = [int(v) for v in subprocess.check_output([str(exe), *args], text=True).split()]
    for (s, p, st, i), want in zip(cases, got):
        assert int(sref.philox_words(s, p, [i], stream=st)[0]) == want, (s, p, st, i)
