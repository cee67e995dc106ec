"""Sampling for the decode step: the reference's parameter structs, logits processor and sampler
(src/sampling/parameters.h, logits_processor.h, sampler.cpp) over ONE fused HIP launch
(csrc/sampling.hip, include/slm_hip.h section 8).

    params = SamplingParameters.create([SamplingParameter(temperature=0.8, top_k=50, top_p=0.9,
                                                           do_sample=True)] * n, device=dev)
    out = sample_logits(logits, params, positions)      # SampleOutput(next_tokens, logprobs, ...)

Differences from the reference, all deliberate (slm_hip.h section 8 states the contract):
  - every ordering is stable by index (the reference's torch sort is not);
  - per-row seeds make sampling reproducible (the reference keeps `seed` "not used for now",
    parameters.h:27-28): a request without one draws it on the host when it is created;
  - the parameters are fp32 tensors (the reference rounds them to the logits dtype first);
  - token ids are int32 (the project's token dtype; the reference returns int64).
Nothing falls back to torch: processing and sampling are HIP kernels.
"""
from __future__ import annotations

import dataclasses
import secrets
from typing import List, Optional, Sequence

import torch

from . import kernels
from ._lib import SLM_SAMPLE_MAX_TOP, SlmError


@dataclasses.dataclass
class SamplingParameter:
    """One request's parameters (parameters.h:13-29), plus a 64-bit seed."""
    frequency_penalty: float = 0.0
    presence_penalty: float = 0.0
    repetition_penalty: float = 1.0
    temperature: float = 0.7
    top_p: float = 1.0
    top_k: int = -1
    logprobs: bool = False
    top_logprobs: int = 0
    do_sample: bool = False
    seed: Optional[int] = None

    def __post_init__(self):
        if self.seed is None:  # drawn once, when the request is created: its tokens are reproducible
            self.seed = secrets.randbits(64)
        self.seed &= (1 << 64) - 1


@dataclasses.dataclass
class SampleOutput:
    """sampling/parameters.h:121-135 (next_tokens int32)."""
    next_tokens: torch.Tensor
    probs: Optional[torch.Tensor] = None
    logprobs: Optional[torch.Tensor] = None
    top_logprobs: Optional[torch.Tensor] = None
    top_tokens: Optional[torch.Tensor] = None


_PARAM_FIELDS = ("frequency_penalties", "presence_penalties", "repetition_penalties", "temperatures", "top_p",
                 "top_k", "unique_token_ids", "unique_token_counts", "unique_token_ids_lens", "do_sample", "seeds")
# the value of a field that is neutral for a row (no penalty, t = 1, top-p / top-k off, no tokens, greedy)
_NEUTRAL = dict(frequency_penalties=0.0, presence_penalties=0.0, repetition_penalties=1.0, temperatures=1.0,
                top_p=1.0, top_k=-1, unique_token_ids=0, unique_token_counts=0, unique_token_ids_lens=0,
                do_sample=False, seeds=0)
# the value of a field that is neutral for a row (no penalty, t = 1, top-p / top-k off, no tokens, greedy)
_NEUTRAL = dict(frequency_penalties=0.0, presence_penalties=0.0, repetition_penalties=1.0, temperatures=1.0,
                top_p=1.0, top_k=-1, unique_token_ids=0, unique_token_counts=0, unique_token_ids_lens=0,
                do_sample=False, seeds=0)


@dataclasses.dataclass
class SamplingParameters:
    """A batch's parameters as device tensors (parameters.h:33-119), one row per sampled sequence.
    A field left None is neutral for every row.  For a captured step, create it once at the maximum
    batch with compact=False (every field materialised) and refresh it in place with copy_() before
    each replay, as the runner refreshes its static inputs."""
    frequency_penalties: Optional[torch.Tensor] = None   # [n] fp32
    presence_penalties: Optional[torch.Tensor] = None    # [n] fp32
    repetition_penalties: Optional[torch.Tensor] = None  # [n] fp32
    temperatures: Optional[torch.Tensor] = None          # [n] fp32
    top_p: Optional[torch.Tensor] = None                 # [n] fp32
    top_k: Optional[torch.Tensor] = None                 # [n] int64
    unique_token_ids: Optional[torch.Tensor] = None      # [n, max_unique] int64
    unique_token_counts: Optional[torch.Tensor] = None   # [n, max_unique] int32
    unique_token_ids_lens: Optional[torch.Tensor] = None  # [n] int32
    do_sample: Optional[torch.Tensor] = None             # [n] bool
    seeds: Optional[torch.Tensor] = None                 # [n] int64 (the uint64 seed's bits)
    logprobs: bool = False
    max_top_logprobs: int = 0

    @classmethod
    def create(cls, params: Sequence[SamplingParameter],
               unique_token_ids: Optional[Sequence[Sequence[int]]] = None,
               unique_token_counts: Optional[Sequence[Sequence[int]]] = None,
               device="cuda", compact: bool = True, max_unique: Optional[int] = None) -> "SamplingParameters":
        """SamplingParameters::init (parameters.cpp) for one row per request.  unique_token_ids[r] /
        unique_token_counts[r]: the distinct tokens of request r so far and how often each occurred."""
        n = len(params)
        dev = torch.device(device)
        ids_l = [list(x) for x in unique_token_ids] if unique_token_ids is not None else [[] for _ in range(n)]
        cnt_l = [list(x) for x in unique_token_counts] if unique_token_counts is not None else \
            [[1] * len(x) for x in ids_l]
        if len(ids_l) != n or len(cnt_l) != n or any(len(a) != len(b) for a, b in zip(ids_l, cnt_l)):
            raise SlmError("unique_token_ids / unique_token_counts do not match the requests")
        mu = max([len(x) for x in ids_l] + [0]) if max_unique is None else int(max_unique)
        f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)  # noqa: E731
        out = cls()
        cols = {
            "frequency_penalties": ([p.frequency_penalty for p in params], 0.0, f32),
            "presence_penalties": ([p.presence_penalty for p in params], 0.0, f32),
            "repetition_penalties": ([p.repetition_penalty for p in params], 1.0, f32),
            "temperatures": ([p.temperature for p in params], None, f32),
            "top_p": ([p.top_p for p in params], 1.0, f32),
            "top_k": ([p.top_k for p in params], -1,
                      lambda v: torch.tensor(v, dtype=torch.int64, device=dev)),
            "do_sample": ([p.do_sample for p in params], False,
                          lambda v: torch.tensor(v, dtype=torch.bool, device=dev)),
        }
        for name, (vals, neutral, make) in cols.items():
            if not compact or neutral is None or any(v != neutral for v in vals):
                setattr(out, name, make(vals))
        out.seeds = torch.tensor([s - (1 << 64) if s >= (1 << 63) else s for s in (p.seed for p in params)],
                                 dtype=torch.int64, device=dev)
        penalised = any(p.frequency_penalty != 0 or p.presence_penalty != 0 or p.repetition_penalty != 1
                        for p in params)
        if mu > 0 and (penalised or not compact):
            ids = torch.zeros(n, mu, dtype=torch.int64)
            cnt = torch.zeros(n, mu, dtype=torch.int32)
            for r, (a, b) in enumerate(zip(ids_l, cnt_l)):
                if len(a) > mu:
                    raise SlmError(f"request {r}: {len(a)} unique tokens > max_unique {mu}")
                ids[r, :len(a)] = torch.tensor(a, dtype=torch.int64)
                cnt[r, :len(b)] = torch.tensor(b, dtype=torch.int32)
            out.unique_token_ids, out.unique_token_counts = ids.to(dev), cnt.to(dev)
            out.unique_token_ids_lens = torch.tensor([len(a) for a in ids_l], dtype=torch.int32, device=dev)
        out.logprobs = any(p.logprobs for p in params)
        out.max_top_logprobs = max([p.top_logprobs for p in params] + [0]) if out.logprobs else 0
        if out.max_top_logprobs > SLM_SAMPLE_MAX_TOP:
            raise SlmError(f"top_logprobs > {SLM_SAMPLE_MAX_TOP}")
        return out

    def narrow(self, n: int) -> "SamplingParameters":
        """The first n rows (views: a captured step at batch n reads the max-batch tensors)."""
        out = dataclasses.replace(self)
        for name in _PARAM_FIELDS:
            t = getattr(self, name)
            if t is not None:
                setattr(out, name, t[:n])
        return out

    def copy_(self, other: "SamplingParameters") -> "SamplingParameters":
        """Refresh rows [0, n) in place (the tensors a captured graph reads) from `other`, a batch of n
        rows created in any form: a field `other` leaves None (neutral for all its rows) is written as
        the neutral value, so nothing of the previous batch survives in rows [0, n)."""
        n = next((getattr(other, f).size(0) for f in _PARAM_FIELDS if getattr(other, f) is not None), None)
        if n is None:
            raise SlmError("copy_ from an empty SamplingParameters")
        for name in _PARAM_FIELDS:
            dst, src = getattr(self, name), getattr(other, name)
            if dst is None:
                if src is not None:
                    raise SlmError(f"{name} was not materialised at creation (compact=False)")
                continue
            if n > dst.size(0) or (src is not None and src.dim() == 2 and src.size(1) > dst.size(1)):
                raise SlmError(f"{name}: a batch of {n} rows does not fit {tuple(dst.shape)}")
            if src is None:
                dst[:n].fill_(_NEUTRAL[name])
            elif src.dim() == 2 and src.size(1) != dst.size(1):
                dst[:n].zero_()
                dst[:n, :src.size(1)].copy_(src)
            else:
                dst[:n].copy_(src)
        self.logprobs, self.max_top_logprobs = other.logprobs, other.max_top_logprobs
        return self

    def processing_kwargs(self) -> dict:
        pen = self.unique_token_ids is not None  # no penalised tokens: the penalties are no-ops
        return dict(frequency_penalties=self.frequency_penalties if pen else None,
                    presence_penalties=self.presence_penalties if pen else None,
                    repetition_penalties=self.repetition_penalties if pen else None,
                    temperatures=self.temperatures, top_k=self.top_k, top_p=self.top_p)


class LogitsProcessor:
    """LogitsProcessor::create(params) (logits_processor.h:89-90): frequency / presence penalties,
    repetition penalty, temperature, top-k / top-p -- as ONE launch, in place."""

    def __init__(self, params: SamplingParameters):
        self.kw = params.processing_kwargs()

    @classmethod
    def create(cls, params: SamplingParameters) -> "LogitsProcessor":
        return cls(params)

    def forward(self, logits: torch.Tensor, unique_token_ids: Optional[torch.Tensor] = None,
                unique_token_counts: Optional[torch.Tensor] = None,
                unique_token_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        kw = dict(self.kw)
        if unique_token_ids is None:
            kw.update(frequency_penalties=None, presence_penalties=None, repetition_penalties=None)
        return kernels.logits_process(logits, unique_token_ids=unique_token_ids,
                                      unique_token_counts=unique_token_counts,
                                      unique_token_lens=unique_token_lens, **kw)

    __call__ = forward


def _outputs(n: int, V: int, device, logprobs: bool, n_top: int, want_probs: bool) -> dict:
    out = {}
    if want_probs:
        out["probs"] = torch.empty(n, V, dtype=torch.float32, device=device)
    if logprobs:
        out["logprobs"] = torch.empty(n, dtype=torch.float32, device=device)
        if n_top > 0:
            out["top_logprobs"] = torch.empty(n, n_top, dtype=torch.float32, device=device)
            out["top_tokens"] = torch.empty(n, n_top, dtype=torch.int32, device=device)
    return out


class Sampler:
    """Sampler(do_sample, logprobs, max_top_logprobs) (sampler.h, sampler.cpp:9-70) on already processed
    logits: greedy rows take the argmax, sampled rows the exponential race argmax(probs / E), E drawn
    from (seeds[r], positions[r]) -- no host synchronisation (the reference's all()/any() reads are
    not needed: every row takes its own path inside the kernel)."""

    def __init__(self, do_sample: torch.Tensor, logprobs: bool = False, max_top_logprobs: int = 0,
                 seeds: Optional[torch.Tensor] = None, positions: Optional[torch.Tensor] = None,
                 want_probs: bool = True):
        self.do_sample, self.logprobs, self.max_top_logprobs = do_sample, logprobs, int(max_top_logprobs)
        self.seeds, self.positions, self.want_probs = seeds, positions, want_probs

    def forward(self, logits: torch.Tensor) -> SampleOutput:
        n, V = logits.shape
        outs = _outputs(n, V, logits.device, self.logprobs, self.max_top_logprobs, self.want_probs)
        tok = kernels.sample(logits, do_sample=self.do_sample, seeds=self.seeds, positions=self.positions, **outs)
        return SampleOutput(tok, **outs)

    __call__ = forward


def sample_logits(logits: torch.Tensor, params: SamplingParameters, positions: Optional[torch.Tensor] = None,
                  want_probs: bool = False, processed: Optional[torch.Tensor] = None,
                  out: Optional[SampleOutput] = None) -> SampleOutput:
    """LogitsProcessor + Sampler fused: one launch for [n_rows, vocab] logits (f16, bf16 or fp32).
    positions[r]: position of row r's last input token (the RNG counter).  `out` supplies static output
    buffers (a captured step); `processed` receives the processed logits."""
    n, V = logits.shape
    if out is None:
        out = SampleOutput(torch.empty(n, dtype=torch.int32, device=logits.device),
                           **_outputs(n, V, logits.device, params.logprobs, params.max_top_logprobs, want_probs))
    kernels.sample(logits, next_tokens=out.next_tokens, positions=positions, do_sample=params.do_sample,
                   seeds=params.seeds, unique_token_ids=params.unique_token_ids,
                   unique_token_counts=params.unique_token_counts, unique_token_lens=params.unique_token_ids_lens,
                   processed=processed, probs=out.probs, logprobs=out.logprobs, top_logprobs=out.top_logprobs,
                   top_tokens=out.top_tokens, **params.processing_kwargs())
    return out


__all__: List[str] = ["SamplingParameter", "SamplingParameters", "SampleOutput", "LogitsProcessor", "Sampler",
                      "sample_logits"]
