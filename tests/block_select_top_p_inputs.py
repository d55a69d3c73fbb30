"""Inputs and grids of the top-p block-selection tests (tests/block_select_top_p_ref.py is the reference), CPU tensors from seeded
generators.  The end-to-end cases are those of tests/block_select_inputs.py, by import; this file adds

  synthetic means   fp32 qbar (1, nbq, 2, 32) and kbar (1, nbk, 1, 32) handed to usp_block_select_top_p directly: N(0, 1) / sqrt(128)
                    -- what pooling 128 rows of white noise gives -- with row block I of q scaled by a factor that grows
                    geometrically from 4 to 32 over the rows, so that at one scale the rows run from flat to peaked.  nbq =
                    min(nbk, 6) rows, placed at row_block0 = 0 or at the end (row_block0 = nbk - nbq).
  two scales        the default D ** -0.5, at which the weights of a row are nearly uniform, and `peaked_scale`: the first of
                    D ** -0.5 * 2 ** k at which, by the fp64 reference, some row of the full-attention selections at top_p 0.05
                    keeps one block and some row at top_p 0.9 keeps at least 70 % of what it sees (nbk >= 5).
  grids             SYNTH_GRID: causal x row_block0 x keep_first {0, 2} x keep_local {1, 2} x top_p {0.05, 0.5, 0.9, 1.0}, share_group
                    alternating; WHITE_GRID: causal x top_p x (keep_first, keep_local) in {(0, 1), (2, 2)} x share_group.
  the ambiguous share of a CASE is taken over all rows of all selections of its grid (tests/block_select_top_p_ref.py: a row is
  ambiguous when another set than the reference's passes the rule)."""
import torch

import block_select_top_p_ref as TR

SYNTH_NBK = (1, 3, 4, 5, 255, 256, 257, 515)
SYNTH_D, SYNTH_HQ, SYNTH_HKV = 32, 2, 1
TOP_PS = (0.05, 0.5, 0.9, 1.0)
CAP = 0.01
PLANTED_SCALE = 16.0       # the planted weights lie 1 / 64 apart: at this scale neighbours differ by a quarter in the exponent
# seeds for which the fp64 reference shows every synthetic case under the cap at both scales (tests/test_block_select_top_p_cpu.py
# asserts it): near-uniform weights over hundreds of blocks lie within a few eps of each other, and of seeds 0..5 these do not
SYNTH_SEED = {255: 5, 256: 2, 257: 3, 515: 4}


def synthetic_means(nbk, seed=None):
    """(qbar (1, nbq, 2, 32), kbar (1, nbk, 1, 32)) fp32."""
    seed = SYNTH_SEED.get(nbk, 0) if seed is None else seed
    g = torch.Generator().manual_seed(7000 + nbk + seed)
    nbq = min(nbk, 6)
    qbar = torch.randn(1, nbq, SYNTH_HQ, SYNTH_D, generator=g) / 128 ** 0.5
    kbar = torch.randn(1, nbk, SYNTH_HKV, SYNTH_D, generator=g) / 128 ** 0.5
    gain = 2.0 ** (2 + 3 * torch.arange(nbq, dtype=torch.float32) / max(nbq - 1, 1))
    return (qbar * gain[None, :, None, None]).contiguous(), kbar.contiguous()


def synth_grid(nbk):
    """(causal, row_block0, keep_first, keep_local, top_p, share_group) of the entry-point tests at nbk key blocks."""
    nbq = min(nbk, 6)
    out = []
    for causal in (True, False):
        for row0 in sorted({0, nbk - nbq}):
            for kf in (0, 2):
                for kl in (1, 2):
                    for p in TOP_PS:
                        out.append((causal, row0, kf, kl, p, len(out) % 2 == 1))
    return out


def peaked_scale(qbar, kbar):
    """The second scale of a synthetic case, from the fp64 reference alone (module docstring)."""
    nbk = kbar.shape[1]
    base = SYNTH_D ** -0.5
    for k in range(1, 16):
        prob = TR.Problem(scale=base * 2.0 ** k, means=(qbar, kbar))
        lo, _ = prob.judge(0.05, False, 0, 0).counts()
        hi, vis = prob.judge(0.9, False, 0, 0).counts()
        if int(lo.min()) == 1 and (nbk < 5 or float((hi.double() / vis).max()) >= 0.7):
            return base * 2.0 ** k
    raise AssertionError(f"no scale of the ladder spreads the counts at nbk = {nbk}")


def white_grid():
    """(causal, keep_first, keep_local, top_p, share_group) of the end-to-end tests."""
    return [(causal, kf, kl, p, share) for causal in (True, False) for (kf, kl) in ((0, 1), (2, 2)) for p in TOP_PS
            for share in (False, True)]


def case_ambiguity(judged_list):
    """The ambiguous share of a case: over all rows of all its selections."""
    amb = sum(int(j.ambiguous().sum()) for j in judged_list)
    rows = sum(j.E.numel() for j in judged_list)
    return amb / rows
