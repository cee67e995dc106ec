"""Compile-time check of the sampling boundary against the reference's OWN header (the pattern of
test_boundary_headers_cpu.py): one translation unit includes src/kernels/sampling/sampling_kernels.h AND
scalellm_amd/csrc/shim/slm_sampling_hip.h and takes the address of the four functions the shim offers.
A declaration that differs in a parameter type makes `&name` ambiguous and the build fails.  The
reference header includes <curand_kernel.h>; a one-line stub declaring curandState_t stands in for it.
invoke_topk_sampling (a curandState_t* interface nothing in the reference calls) is not offered.
Skipped where the reference tree is absent."""
import os
import subprocess
import sysconfig

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"

TU = r"""
#include "kernels/sampling/sampling_kernels.h"
#include "slm_sampling_hip.h"

auto p1 = &llm::kernel::apply_temperature_penalty;
auto p2 = &llm::kernel::apply_repetition_penalty;
auto p3 = &llm::kernel::apply_frequency_presence_penalty;
auto p4 = &llm::kernel::invoke_softmax;
int main() { return 0; }
"""


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "kernels", "sampling", "sampling_kernels.h")),
                    reason="the reference tree is not mounted here")
@pytest.mark.timeout(600)
def test_sampling_shim_declarations_agree_with_the_reference_header(tmp_path):
    import torch
    from torch.utils import cpp_extension as ce
    stub = tmp_path / "stub"
    stub.mkdir()
    (stub / "curand_kernel.h").write_text("#pragma once\ntypedef struct curandStateXORWOW curandState_t;\n")
    src = tmp_path / "sampling_tu.cpp"
    src.write_text(TU)
    inc = [f"-I{p}" for p in ce.include_paths()] + [f"-I{sysconfig.get_paths()['include']}", f"-I{REF}",
                                                    f"-I{stub}",
                                                    f"-I{os.path.join(ROOT, 'scalellm_amd', 'csrc', 'shim')}",
                                                    f"-I{os.path.join(ROOT, 'include')}"]
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-w",
           f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}", *inc, str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    # the check has teeth: a deliberately wrong redeclaration must fail
    bad = tmp_path / "sampling_bad.cpp"
    bad.write_text(TU.replace('#include "slm_sampling_hip.h"', '#include "slm_sampling_hip.h"\n'
                              'namespace llm::kernel { void apply_temperature_penalty(torch::Tensor&, '
                              'const torch::Tensor&, int extra = 0); }'))
    r2 = subprocess.run(cmd[:-1] + [str(bad)], capture_output=True, text=True)
    assert r2.returncode != 0 and "apply_temperature_penalty" in r2.stderr
