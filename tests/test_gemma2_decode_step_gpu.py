"""Gemma2DecodeStep on an unquantised bf16 checkpoint (quant_method "none", loaded from HuggingFace's names) against
the fp32 PyTorch Gemma-2 of tests/gemma2_decode_case.py: three decode steps of two sequences over a paged cache that
already holds 20 tokens -- more than the window of 16, which layer 0 applies and layer 1 does not.  Compared: the
capped logits of every step and the K / V rows every layer appends.

The cache is prefilled with the reference's K / V of the first 20 tokens, rounded to bf16.  In layer 0 the rows no
step may see (positions 0 .. 4: the first step's window starts at 21 - 16 = 5, inside the first 8-token page) hold
NaN instead, as does every slot no sequence owns: a kernel that loads rows in front of the window and masks them
afterwards turns the whole output into NaN.

Bounds: twice the error of a bf16 framework run of the same model on the same seed (gemma2_decode_case.TOL_*;
tests/test_gemma2_decode_ref_cpu.py shows the bound sees the window, one key more and one key fewer)."""
import pytest
import torch

from tests import gemma2_decode_case as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
BLOCK = 8
BLOCKS_PER_SEQ = (C.PREFILL + C.N_DECODE + BLOCK - 1) // BLOCK


@pytest.fixture(scope="module")
def run():
    from scalellm_amd.gemma2 import Gemma2DecodeStep, Gemma2Shape
    from scalellm_amd.layers import InputParameters
    sd, toks = C.checkpoint(), C.tokens()
    want_logits, want_new, old = C.decode_rows(sd, toks)
    n_blocks = C.N_SEQS * BLOCKS_PER_SEQ + 3
    model = Gemma2DecodeStep(Gemma2Shape.from_hf_config(C.HF_CONFIG), C.N_SEQS, n_blocks, BLOCK, quant_method="none",
                             dtype=torch.bfloat16, device=DEV, seed=1)
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(C.SEED + 2)
    pages = torch.randperm(n_blocks, generator=g)[:C.N_SEQS * BLOCKS_PER_SEQ].view(C.N_SEQS, BLOCKS_PER_SEQ)
    pos = torch.arange(C.PREFILL + C.N_DECODE)
    slots = pages[:, pos // BLOCK] * BLOCK + pos % BLOCK                       # [N_SEQS, positions]
    first_seen = C.PREFILL + 1 - C.HF_CONFIG["sliding_window"]
    for li, L in enumerate(model.layers):
        for cache, rows in zip(L["kv"].get_kv_cache(), old[li]):
            cache.fill_(float("nan"))
            rows = rows.clone()
            if li % 2 == 0:
                rows[:, :first_seen] = float("nan")
            cache[slots[:, :C.PREFILL].reshape(-1).to(DEV)] = rows.flatten(0, 1).to(DEV, torch.bfloat16)
    i32 = lambda x: torch.as_tensor(x, dtype=torch.int32).to(DEV)  # noqa: E731
    got_logits = []
    for t in range(C.N_DECODE):
        p = C.PREFILL + t
        params = InputParameters(q_cu_seq_lens=i32(range(C.N_SEQS + 1)),
                                 kv_cu_seq_lens=i32([s * (p + 1) for s in range(C.N_SEQS + 1)]),
                                 new_cache_slots=i32(slots[:, p]), block_tables=i32((pages * BLOCK).reshape(-1)),
                                 cu_block_lens=i32([s * BLOCKS_PER_SEQ for s in range(C.N_SEQS + 1)]),
                                 q_max_seq_len=1, kv_max_seq_len=p + 1)
        logits = model.forward(i32(toks[:, p]), i32([p] * C.N_SEQS), params, return_logits=True)
        torch.cuda.synchronize()
        got_logits.append(logits.float().cpu())
    new_slots = slots[:, C.PREFILL:].t().reshape(-1).to(DEV)                    # step-major, as want_new
    got_new = [tuple(cache[new_slots].float().cpu().view_as(want_new[li][x])
                     for x, cache in enumerate(L["kv"].get_kv_cache())) for li, L in enumerate(model.layers)]
    return torch.stack(got_logits), got_new, want_logits, want_new


def test_decode_step_logits_match_the_fp32_reference(run):
    got, _, want, _ = run
    assert got.shape == want.shape and not torch.isnan(got).any()
    for t in range(C.N_DECODE):
        print(f"\n[gemma2-decode] step {t}: logits rel L2 {C.rel_l2(got[t], want[t]):.3e}")
    err = C.rel_l2(got, want)
    print(f"\n[gemma2-decode] logits rel L2 {err:.3e} (bf16 framework run {C.BF16_LOGITS_ERR:.3e}, "
          f"bound {C.TOL_LOGITS:.3e})")
    assert err <= C.TOL_LOGITS
    assert float(got.abs().max()) <= C.HF_CONFIG["final_logit_softcapping"]


def test_decode_step_appends_the_reference_keys_and_values(run):
    _, got, _, want = run
    cat = lambda new, x: torch.cat([layer[x] for layer in new])  # noqa: E731
    for li in range(len(want)):
        print(f"\n[gemma2-decode] layer {li}: K rel L2 {C.rel_l2(got[li][0], want[li][0]):.3e}, "
              f"V rel L2 {C.rel_l2(got[li][1], want[li][1]):.3e}")
    for x, name, recorded, tol in ((0, "K", C.BF16_K_ERR, C.TOL_K), (1, "V", C.BF16_V_ERR, C.TOL_V)):
        assert not torch.isnan(cat(got, x)).any(), name
        err = C.rel_l2(cat(got, x), cat(want, x))
        print(f"\n[gemma2-decode] appended {name} rel L2 {err:.3e} (bf16 framework run {recorded:.3e}, "
              f"bound {tol:.3e})")
        assert err <= tol, name


def test_only_an_unquantised_step_loads_a_state_dict():
    from scalellm_amd.gemma2 import Gemma2DecodeStep, Gemma2Shape
    model = Gemma2DecodeStep(Gemma2Shape.from_hf_config(C.HF_CONFIG), 2, 4, BLOCK, quant_method="awq", device=DEV)
    with pytest.raises(ValueError):
        model.load_state_dict(C.checkpoint())
