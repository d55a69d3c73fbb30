"""The fp64 reference of the antidiagonal block weights (include/usp_hip.h: usp_block_antidiag_weights), the plain definition on
the device of its inputs, and the top-p cut over given weights in exact arithmetic.  The tolerance of the weights is derived, in
the form and with the constants of tests/block_mass_ref.py (all terms are non-negative, so it is relative):
    |got - ref| <= ref * (expm1(2 d) + (2 + T) E_EXP + (17 T + 4 + DEPTH) 2^-24 + 2^-23) + FLUSH
  d      the error of one exponent per (batch, head): the MFMA chain over s Dp terms, 2 (scale / s) (s Dp) 2^-24 max sum_(t,d) |q| |k|;
         the expression fma(chain, c, -lse2), K_ROUND u (max |a| + max |lse|) (scale / s is exact); 4 u (max |a| + max |lse|) for the
         kernel's own lse2 = M + log2(L) (v_log_f32 to 2 ulp, one addition).  TWICE: in p and through L, a sum of such exponentials;
  E_EXP  twice v_exp_f32's measured error: for p, for the terms of L, and per tile of sub-columns, T = ceil(ceil(S / s) / 32), for
         the rescaling l * exp2(m - m');   2^-24 per summation step: 17 per tile and 3 for the halves in L; in the block sum
         DEPTH = 16 / (s / 4) lane terms + 1 (halves) + log2(128 / s) (butterfly) + 1 (division);   FLUSH  as there."""
import math
from fractions import Fraction

import torch

import block_mass_ref as MR


def sub_scores(q, k, scale, stride, causal=False):
    """(B, Hq, n_sub, n_sub) fp64: a[r, c], under `causal` -inf where c > r."""
    B, S, Hq, D = q.shape
    n_sub = (S + stride - 1) // stride
    pad = (0, 0, 0, 0, 0, n_sub * stride - S)
    q64 = torch.nn.functional.pad(q.to(torch.float64), pad).view(B, n_sub, stride, Hq, D).flip(2)   # [r, t] = q[r s + s-1-t]
    k64 = torch.nn.functional.pad(k.to(torch.float64), pad).view(B, n_sub, stride, -1, D).repeat_interleave(Hq // k.shape[2], dim=3)
    a = torch.einsum("brthd,bcthd->bhrc", q64, k64) * (scale / stride)
    i = torch.arange(n_sub, device=q.device)
    return a.masked_fill(i[None, :] > i[:, None], float("-inf")) if causal else a


def weights_ref(q, k, scale, causal, stride):
    """(B, Hq, nb, nb) fp64."""
    p = torch.softmax(sub_scores(q, k, scale, stride, causal), dim=-1)
    B, Hq, n_sub, _ = p.shape
    nb, n = (q.shape[1] + 127) // 128, 128 // stride
    p = torch.nn.functional.pad(p, (0, nb * n - n_sub, 0, nb * n - n_sub))
    rows = torch.tensor([min(n, n_sub - I * n) for I in range(nb)], dtype=torch.float64, device=q.device)
    return p.view(B, Hq, nb, n, nb, n).sum(dim=(3, 5)) / rows[None, None, :, None]


def check(got, q, k, scale, causal, stride, what=""):
    """Asserts the bound against weights_ref; prints the largest error as a share of it first."""
    ref, S = weights_ref(q, k, scale, causal, stride), q.shape[1]
    a = sub_scores(q, k, scale, stride)
    pairs = sub_scores(q.to(torch.float64).abs(), k.to(torch.float64).abs(), float(stride), stride).amax(dim=(-1, -2))   # sum_(t,d) |q| |k|
    lmax = torch.logsumexp(sub_scores(q, k, scale, stride, causal), dim=-1).abs().amax(dim=-1)
    d = 2.0 * abs(scale) * MR.kernel_head_dim(q.shape[3]) * 2.0 ** -24 * pairs + (MR.K_ROUND + 4) * 2.0 ** -24 * (a.abs().amax(dim=(-1, -2)) + lmax)
    T = ((S + stride - 1) // stride + 31) // 32
    depth = 16 // (stride // 4) + 1 + int(math.log2(128 // stride)) + 1
    tol = ref * (torch.expm1(2 * d)[..., None, None] + (2 + T) * MR.E_EXP + (17 * T + 4 + depth) * 2.0 ** -24 + 2.0 ** -23) + MR.FLUSH
    got = got.detach().to(ref.device).to(torch.float64)
    assert got.shape == ref.shape and not torch.isnan(got).any(), what
    share = float(((got - ref).abs() / tol).max())
    print(f"ANTIDIAGERR {what} {share:.3f} of the bound (largest |err| {float((got - ref).abs().max()):.3e}, d {float(d.max()):.2e})")
    assert share <= 1.0, f"{what}: {share:.3f} x the bound"


def select_from_weights_ref(w, top_p, causal, keep_first, keep_local, row_block0=0):
    """The mask of include/usp_hip.h: usp_block_select_weights in exact arithmetic, for weights whose every partial sum is exact in
    fp32 (dyadic rationals: then SUM's order and the fmaf are exact too): (B, Hq, nbq, nbk) bool."""
    nbk = w.shape[3]
    out = torch.zeros(w.shape, dtype=torch.bool)
    p = torch.tensor(top_p, dtype=torch.float32)
    for b, h, I in ((b, h, I) for b in range(w.shape[0]) for h in range(w.shape[1]) for I in range(w.shape[2])):
        row, Ig = [Fraction(float(x)) for x in w[b, h, I]], row_block0 + I
        nv = min(Ig + 1, nbk) if causal else nbk
        forced = [J < nv and (J < keep_first or Ig - keep_local < J <= Ig) for J in range(nbk)]
        target = Fraction(float(p * torch.tensor(float(sum(row)), dtype=torch.float32)))      # the kernel's one fp32 product
        have = sum(x for x, f in zip(row, forced) if f)
        out[b, h, I] = torch.tensor(forced)
        for J in sorted((J for J in range(nv) if not forced[J]), key=lambda J: (-row[J], J)):
            if have >= target:
                break
            out[b, h, I, J] = True
            have += row[J]
    return out
