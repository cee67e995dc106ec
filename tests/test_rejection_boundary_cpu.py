"""The shim's slm::RejectionSampler (scalellm_amd/csrc/shim/slm_rejection_sampler_hip.h) against the reference's
llm::RejectionSampler (src/speculative/rejection_sampler.h), checked TEXTUALLY in the manner of
test_boundary_interfaces_cpu.py: every method of the reference class -- the constructor, forward,
build_accepted_mask, random_sample and greedy_sample -- exists in the shim with the same return type, the same
static / const qualifiers and the same parameter types in the same order.  The shim may only append parameters
that carry a default (the per-sequence seeds and positions).  Skipped where the reference tree is absent."""
import os
import re

import pytest

from tests.test_boundary_interfaces_cpu import REF, SHIM, _class_body, _param_type, _split_top, _strip_comments

METHODS = ("RejectionSampler", "forward", "build_accepted_mask", "random_sample", "greedy_sample")


def _methods(text):
    body = _strip_comments(_class_body(text, "RejectionSampler"))
    out = {}
    for m in re.finditer(r"(?<![>.\w])(" + "|".join(METHODS) + r")\s*\(", body):
        name = m.group(1)
        if name in out:
            continue
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(body[i], 0)
            i += 1
        head = body[:m.start()]
        head = head[max(head.rfind(";"), head.rfind("}"), head.rfind(":") if name == "RejectionSampler" else -1,
                        head.rfind("public:"), head.rfind("{")) + 1:]
        head = re.sub(r"\b(public|private)\s*:", " ", head)
        static = bool(re.search(r"\bstatic\b", head))
        ret = " ".join(re.sub(r"\bstatic\b", " ", head).split())
        raw = [p for p in _split_top(body[m.end():i - 1]) if p.strip()]
        params = [_param_type(p) for p in raw]
        defaults = ["=" in p for p in raw]
        const = bool(re.match(r"\s*const\b", body[i:i + 12]))
        out[name] = dict(ret=ret.split("::")[-1] if ret.endswith("SampleOutput") else ret, static=static,
                         params=params, defaults=defaults, const=const)
    return out


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "speculative", "rejection_sampler.h")),
                    reason="the reference tree is not mounted here")
def test_rejection_sampler_declares_the_reference_methods():
    with open(os.path.join(REF, "speculative", "rejection_sampler.h")) as f:
        ref = _methods(f.read())
    with open(os.path.join(SHIM, "slm_rejection_sampler_hip.h")) as f:
        ours = _methods(f.read())
    assert set(ref) == set(METHODS), ref
    assert ref["random_sample"]["static"] and not ref["forward"]["static"] and ref["forward"]["const"]
    for name, r in ref.items():
        o = ours.get(name)
        assert o is not None, f"slm::RejectionSampler lacks {name}"
        assert (o["ret"], o["static"], o["const"]) == (r["ret"], r["static"], r["const"]), (name, o, r)
        n = len(r["params"])
        assert o["params"][:n] == r["params"], (name, o["params"], r["params"])
        assert all(o["defaults"][n:]), f"{name}: appended parameters must carry defaults"
        assert o["defaults"][:n] == r["defaults"], (name, "default arguments differ")
    # the optional trailing arguments are the seeds and positions tensors
    assert ours["RejectionSampler"]["params"][3:] == ["const torch::Tensor&"] * 2
    assert ours["random_sample"]["params"][6:] == ["const torch::Tensor&"] * 2
