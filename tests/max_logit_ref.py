"""The reference of `return_max_logits` (include/usp_hip.h: usp_flash_fwd_maxlogit), dense and small, in fp64:

    row_max[b, h, i] = max over the keys j row i SEES of  softmax_scale * q[b, i, h] . k[b, j, h // G]      (-inf: none)
    max_logits[h]    = max over b, i of row_max[b, h, i]

on the 16-bit operands as given.  The visible set is tests/shift_ref.py's (`visible`: causal, ragged Sk, window, shift), shared
with the windowed-ring tests, not re-derived here.

The tolerance is derived, not chosen.  A product of two 16-bit operands is exact in fp32, so what separates the kernel's score
from the exact one is the fp32 accumulation over the Dp terms of the MFMA chain (Dp: the head dim the kernel runs at; the zero
padding adds exact zeros) and ONE rounding of the product by softmax_scale:

    |got - ref| <= 2 * scale * Dp * 2^-24 * max_pairs sum_d |q_d k_d|  +  2^-23 |ref|

the factor 2 covering the MFMA's internal summation order -- the form tests/test_gpu_sink.py uses for `delta`.  The maximum is
monotone, so a bound that holds for every score holds for the maximum of any subset.  `abs_pairs` is taken over ALL pairs of a
(batch, head), visible or not: an upper bound of the visible ones, cheaper, and still ~1e-5 at D = 128 on N(0, 1) inputs."""
import torch

from oracle_backend import OracleBlockBackend
from shift_ref import visible


def _scores(q, k, scale, causal=False, window=None, shift=0):
    """(masked scores (B,Hq,Sq,Sk) fp64, sum_d |q_d k_d| of every pair, same shape)"""
    G = q.shape[2] // k.shape[2]
    q64 = q.to(torch.float64)
    k64 = k.to(torch.float64).repeat_interleave(G, dim=2)
    s = torch.einsum("bihd,bjhd->bhij", q64, k64) * scale
    a = torch.einsum("bihd,bjhd->bhij", q64.abs(), k64.abs())
    vis = visible(q.shape[1], k.shape[1], causal, window, shift, q.device)
    return s.masked_fill(~vis, float("-inf")), a


def row_max_ref(q, k, scale, causal=False, window=None, shift=0):
    """(B, Hq, Sq) fp64 on q's device; -inf where a row sees nothing."""
    return _scores(q, k, scale, causal, window, shift)[0].amax(dim=-1)


def max_logits_ref(q, k, scale, causal=False, window=None, shift=0):
    """(Hq,) fp64."""
    return row_max_ref(q, k, scale, causal, window, shift).amax(dim=(0, 2))


def abs_pairs(q, k):
    """(B, Hq) fp64: max over the pairs (i, j) of sum_d |q_d k_d|, per batch and head."""
    return _scores(q, k, 1.0)[1].amax(dim=(-1, -2))


def tolerance(ref, scale, Dp, pairs):
    """The bound above, elementwise on `ref` ((B, Hq, Sq) with `pairs` (B, Hq), or (Hq,) with pairs.amax(0)); infinite where the
    reference is -inf (there the value must be -inf exactly: `check`)."""
    p = pairs[..., None] if ref.dim() == 3 else pairs
    return 2.0 * scale * Dp * 2.0 ** -24 * p + 2.0 ** -23 * ref.abs()


def check(got, ref, scale, Dp, pairs, what=""):
    """Asserts the bound; prints the largest error as a fraction of it first.  -inf must be -inf.  Returns that fraction."""
    got = got.to(torch.float64)
    empty = torch.isinf(ref) & (ref < 0)
    assert torch.equal(torch.isinf(got) & (got < 0), empty), f"{what}: -inf exactly where nothing is visible"
    assert not torch.isnan(got).any(), f"{what}: NaN"
    tol = tolerance(ref, scale, Dp, pairs)
    err = torch.where(empty, torch.zeros_like(ref), (got - ref).abs())
    frac = float((err / torch.where(empty, torch.ones_like(tol), tol)).max())
    print(f"MAXLERR {what} {frac:.3f} of the bound (largest |err| {float(err.max()):.3e})")
    assert frac <= 1.0, f"{what}: {frac:.3f} x the bound"
    return frac


class MaxLogitOracleBackend(OracleBlockBackend):
    """The CPU oracle backend serving `row_max=` (and row_max_reduce), for the orchestration tests: the launch that opens a row
    range writes the fp64 row maxima of its block, a merging launch takes the maximum with what is there.  `row_max_calls`
    records them apart, so `calls` stays what the base class records."""

    def __init__(self):
        super().__init__()
        self.row_max_calls = []

    def fwd(self, q, k, v, softmax_scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None,
            row_max=None, **kw):
        # cooperative (`super().fwd`), so it also sits in front of an oracle that takes `shift` (the windowed ring's)
        super().fwd(q, k, v, softmax_scale, causal, lse, out, acc, merge_in, final_begin, final_end, **kw)
        if row_max is None:
            return
        assert row_max.dtype == torch.float32 and row_max.shape == lse.shape and (row_max.stride(-1) == 1 or row_max.shape[-1] == 1)
        self.row_max_calls.append(("fwd", tuple(q.shape), tuple(k.shape), bool(causal), bool(merge_in)))
        rm = row_max_ref(q, k, softmax_scale, causal, kw.get("window"), kw.get("shift") or 0).to(torch.float32)
        row_max.copy_(torch.maximum(row_max, rm) if merge_in else rm)

    def row_max_reduce(self, row_max, out=None, accum=False):
        self.row_max_calls.append(("reduce", tuple(row_max.shape), bool(accum)))
        r = row_max.amax(dim=(0, 2))
        if out is None:
            return r
        out.copy_(torch.maximum(out, r) if accum else r)
        return out
