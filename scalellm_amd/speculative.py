"""Validation of speculative drafts: the reference's RejectionSampler (src/speculative/rejection_sampler.h,
rejection_sampler.cpp) over the two-launch HIP kernel (csrc/rejection.hip, include/slm_hip.h section 9).

    rs = RejectionSampler(do_sample, logprobs=False, max_top_logprobs=0, seeds=seeds, positions=positions)
    out = rs.forward(draft_token_ids, draft_probs, target_logits, bonus_token_ids, mask_out_rejected_tokens=True)
    out.next_tokens       # int32 [n_seqs, k + 1], -1 after the first rejected row
    out.accepted_lens     # int32 [n_seqs]: verify-row inputs whose KV entries stay valid

Differences from the reference, all deliberate (slm_hip.h section 9 states the contract):
  - no host synchronisation: the constructor does not read do_sample (the reference's all() / any(),
    rejection_sampler.cpp:28-29); every sequence takes its own path inside the kernel, so the call can
    be captured in a graph;
  - the acceptance draw and the recovery race are seeded Philox (streams 1 and 2 of slm_sample's
    counter), keyed by each sequence's seed and the position of its row-0 input token, instead of
    unseeded torch::rand / exponential_;
  - token ids are int32 (the project's token dtype; the reference returns int64);
  - SampleOutput.accepted_lens is an addition.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Tuple

import torch

from . import kernels
from ._lib import SLM_SAMPLE_MAX_TOP, SlmError
from .sampling import SampleOutput


@dataclasses.dataclass
class RejectionOutput(SampleOutput):
    """SampleOutput (next_tokens [n, k + 1], logprobs [n, k + 1], top_* [n, k + 1, n_top]) plus the accepted
    lengths [n] (first rejected row + 1)."""
    accepted_lens: Optional[torch.Tensor] = None


def _validate(draft_token_ids, draft_probs, target, bonus_token_ids, *, target_is_probs, mask, do_sample=None,
              seeds=None, positions=None, uniform=None, logprobs=False, n_top=0,
              out: Optional[RejectionOutput] = None) -> RejectionOutput:
    n, k = draft_token_ids.shape
    dev = target.device
    if out is None:
        out = RejectionOutput(torch.empty(n, k + 1, dtype=torch.int32, device=dev),
                              accepted_lens=torch.empty(n, dtype=torch.int32, device=dev))
        if logprobs:
            out.logprobs = torch.empty(n, k + 1, dtype=torch.float32, device=dev)
            if n_top > 0:
                out.top_logprobs = torch.empty(n, k + 1, n_top, dtype=torch.float32, device=dev)
                out.top_tokens = torch.empty(n, k + 1, n_top, dtype=torch.int32, device=dev)
    kernels.rejection_sample(draft_token_ids, draft_probs, target, bonus_token_ids.reshape(-1),
                             target_is_probs=target_is_probs, mask_out_rejected=mask, do_sample=do_sample,
                             seeds=seeds, positions=positions, uniform=uniform, next_tokens=out.next_tokens,
                             accepted_lens=out.accepted_lens, logprobs=out.logprobs, top_logprobs=out.top_logprobs,
                             top_tokens=out.top_tokens)
    return out


class RejectionSampler:
    """RejectionSampler(do_sample, logprobs, max_top_logprobs) (rejection_sampler.h:9-64) plus per-sequence
    seeds and positions.  positions[s]: the position of the input token of sequence s's row 0 (row j draws
    with positions[s] + j)."""

    def __init__(self, do_sample: torch.Tensor, logprobs: bool = False, max_top_logprobs: int = 0,
                 seeds: Optional[torch.Tensor] = None, positions: Optional[torch.Tensor] = None):
        if int(max_top_logprobs) > SLM_SAMPLE_MAX_TOP:
            raise SlmError(f"max_top_logprobs > {SLM_SAMPLE_MAX_TOP}")
        self.do_sample, self.logprobs, self.max_top_logprobs = do_sample, bool(logprobs), int(max_top_logprobs)
        self.seeds, self.positions = seeds, positions

    def forward(self, draft_token_ids: torch.Tensor, draft_probs: Optional[torch.Tensor],
                target_logits: torch.Tensor, bonus_token_ids: torch.Tensor,
                mask_out_rejected_tokens: bool = False, out: Optional[RejectionOutput] = None) -> RejectionOutput:
        """draft_token_ids [n, k]; draft_probs [n, k, V] fp32; target_logits [n, k + 1, V]; bonus_token_ids
        [n] or [n, 1].  next_tokens: [n, k + 1], masked with -1 after the first rejection if asked.
        logprobs are taken at the unmasked tokens, as the reference takes them."""
        return _validate(draft_token_ids, draft_probs, target_logits, bonus_token_ids, target_is_probs=False,
                         mask=mask_out_rejected_tokens, do_sample=self.do_sample, seeds=self.seeds,
                         positions=self.positions, logprobs=self.logprobs,
                         n_top=self.max_top_logprobs if self.logprobs else 0, out=out)

    __call__ = forward

    @staticmethod
    def build_accepted_mask(accepted: torch.Tensor) -> torch.Tensor:
        """[n, k] accepted -> [n, k + 1] bool: True up to and including the first rejected row
        (rejection_sampler.cpp:118-141)."""
        n, k = accepted.shape
        rejected = torch.cat([~accepted.bool(), torch.ones(n, 1, dtype=torch.bool, device=accepted.device)], dim=1)
        first = rejected.int().argmax(dim=1, keepdim=True)  # the first True: argmax returns the first maximum
        return torch.arange(k + 1, device=accepted.device).unsqueeze(0) <= first

    @staticmethod
    def random_sample(draft_token_ids: torch.Tensor, draft_probs: torch.Tensor, target_probs: torch.Tensor,
                      uniform_rand: Optional[torch.Tensor], bonus_token_ids: torch.Tensor,
                      mask_out_rejected_tokens: bool, seeds: Optional[torch.Tensor] = None,
                      positions: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """rejection_sampler.cpp:143-190 on fp32 target probabilities [n, k, V]: (tokens, masked tokens or None).
        uniform_rand [n, k] replaces the acceptance draw; the recovery race draws from seeds / positions."""
        n = draft_token_ids.size(0)
        do = torch.ones(n, dtype=torch.bool, device=draft_token_ids.device)
        return RejectionSampler._pair(draft_token_ids, draft_probs, target_probs, bonus_token_ids,
                                      mask_out_rejected_tokens, do, seeds, positions, uniform_rand)

    @staticmethod
    def greedy_sample(draft_token_ids: torch.Tensor, target_probs: torch.Tensor, bonus_token_ids: torch.Tensor,
                      mask_out_rejected_tokens: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """rejection_sampler.cpp:192-224 on fp32 target probabilities [n, k, V]: (tokens, masked tokens or None)."""
        return RejectionSampler._pair(draft_token_ids, None, target_probs, bonus_token_ids,
                                      mask_out_rejected_tokens, None, None, None, None)

    @staticmethod
    def _pair(draft_token_ids, draft_probs, target_probs, bonus_token_ids, mask, do_sample, seeds, positions,
              uniform):
        out = _validate(draft_token_ids, draft_probs, target_probs, bonus_token_ids, target_is_probs=True,
                        mask=False, do_sample=do_sample, seeds=seeds, positions=positions, uniform=uniform)
        masked = None
        if mask:  # every entry after the first rejected row (accepted_lens - 1) becomes -1
            k1 = out.next_tokens.size(1)
            keep = torch.arange(k1, device=out.next_tokens.device).unsqueeze(0) < out.accepted_lens.unsqueeze(1)
            masked = torch.where(keep, out.next_tokens, torch.full_like(out.next_tokens, -1))
        return out.next_tokens, masked


__all__: List[str] = ["RejectionSampler", "RejectionOutput"]
