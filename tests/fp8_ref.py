"""Reference and error bound of the e4m3 forward (include/usp_hip.h: USP_ATTN_FP8) and of quantize_fp8.

The reference is exact attention in fp64 on the DEQUANTIZED operands, from the definition: x8.double() * descale is exact.

The element-wise bound of `out` follows the contract, term by term (p = the true probabilities, v the dequantized values, A_id =
sum_j p_ij |v_jd|, l'_i = sum_j exp(s_ij - max_j s_ij) >= 1, n_i = keys row i sees):
  1. P is rounded to e4m3 (3 mantissa bits, round to nearest even) after a multiplication by 2^8, against the RUNNING maximum.
     A normal value moves by at most 2^-4 of itself: 2^-4 A_id.  A subnormal one (2^8 p' < 2^-6) moves by at most half the step
     2^-9, i.e. 2^-10 / 2^8 in units of p' = exp(s - running max); a running maximum below the final one only shrinks that in final
     units, and the division by the row sum turns p' into p: 2^-18 sum_j |v_jd| / l'_i over the visible keys.  The row sum is taken
     from the fp32 values, so it contributes nothing here.  (A merged two-call result obeys the same bound: each call's terms
     are weighted by its share of the row sum, which is at most its own.)
  2. fp32 chains: a score is a sum of D exact products, error <= D 2^-24 scale sum_d |q_id k_jd| =: ds_i (its maximum over j) in
     the exponent; the exponent's FMA and v_exp_f32 add 2^-19 relative at |exponent| <= 32 (anything smaller rounds to zero in
     e4m3 and is covered by 1.); row sum and value product accumulate n_i terms each: (2 (ds_i + 2^-19) + 2 n_i 2^-24) A_id.
  3. The output type rounds the result once: 2^-9 (bf16) or 2^-12 (fp16, + its subnormal step 2^-25) of |out|, taken on ref + 1. + 2.
`lse` never sees the rounded P: it is held to the project's 2e-3 relative / 1e-4 absolute."""
import torch

E4M3_MAX = 448.0


def quantize_cpu(x, per_head_scale=None):
    """fp32 (B, S, H, D) -> (x8 e4m3fn, descale fp32 (B, H)) on the CPU; `per_head_scale` (H,) multiplies x first so that the heads'
    descales differ."""
    x = x.float() * (1.0 if per_head_scale is None else torch.as_tensor(per_head_scale, dtype=torch.float32)[None, None, :, None])
    descale = x.abs().amax(dim=(1, 3)) / E4M3_MAX
    descale = torch.where(descale > 0, descale, torch.ones_like(descale))
    return (x / descale[:, None, :, None]).to(torch.float8_e4m3fn), descale


def attention(q8, k8, v8, dq, dk, dv, scale, causal, out_dtype=torch.bfloat16, shift=0):
    """(out fp64 (B, Sq, Hq, D), lse fp64 (B, Hq, Sq), bound fp64 like out) of the dequantized operands."""
    B, Sq, Hq, D = q8.shape
    Sk, Hkv = k8.shape[1], k8.shape[2]
    g = Hq // Hkv
    q = q8.double() * dq.double()[:, None, :, None]
    k = (k8.double() * dk.double()[:, None, :, None]).repeat_interleave(g, dim=2)
    v = (v8.double() * dv.double()[:, None, :, None]).repeat_interleave(g, dim=2)
    s = torch.einsum("bthd,bshd->bhts", q, k) * scale
    sabs = torch.einsum("bthd,bshd->bhts", q.abs(), k.abs()) * scale
    vis = torch.ones(Sq, Sk, dtype=torch.bool)
    if causal:
        vis = torch.arange(Sk)[None, :] <= torch.arange(Sq)[:, None] + (Sk - Sq + shift)
    s = s.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, -1)
    empty = ~vis.any(-1)                                     # (Sq,)
    lse[:, :, empty] = float("-inf")
    p = torch.nan_to_num(torch.exp(s - lse[..., None]))
    out = torch.einsum("bhts,bshd->bthd", p, v)
    A = torch.einsum("bhts,bshd->bthd", p, v.abs())
    V1 = torch.einsum("ts,bshd->bthd", vis.double(), v.abs())
    lp = torch.nan_to_num(torch.exp(lse - s.amax(-1))).clamp(min=1.0).transpose(1, 2)[..., None]      # l'_i
    ds = (D * 2.0 ** -24 * sabs.masked_fill(~vis, 0.0).amax(-1)).transpose(1, 2)[..., None]
    n = vis.sum(-1).double()[None, :, None, None]
    bound = 2.0 ** -4 * A + 2.0 ** -18 * V1 / lp + (2 * (ds + 2.0 ** -19) + 2 * n * 2.0 ** -24) * A
    r = 2.0 ** -9 if out_dtype == torch.bfloat16 else 2.0 ** -12
    bound = bound + r * (out.abs() + bound) + (2.0 ** -25 if out_dtype == torch.float16 else 0.0)
    return out, lse, bound


def check(out, lse, ref, ref_lse, bound, what=""):
    """out within the bound everywhere, lse within 2e-3 / 1e-4, empty rows exactly 0 / -inf; returns the worst error as a fraction
    of the bound (printed by the tests: measured, not asserted)."""
    out, lse = out.double().cpu(), lse.double().cpu()
    fin = torch.isfinite(ref_lse)
    assert torch.isfinite(out).all(), f"{what}: out has a non-finite element"
    assert (lse[~fin] == float("-inf")).all() and torch.isfinite(lse[fin]).all(), f"{what}: empty rows must give lse = -inf"
    assert (out[~fin.transpose(1, 2)] == 0).all(), f"{what}: empty rows must give out = 0"
    err = (out - ref).abs()
    frac = (err / bound.clamp(min=1e-300))[bound > 0].max().item() if (bound > 0).any() else 0.0
    print(f"{what}: worst out error / bound = {frac:.3f}, worst |lse error| = {(lse[fin] - ref_lse[fin]).abs().max().item() if fin.any() else 0:.2e}")
    assert (err <= bound).all(), f"{what}: out leaves the bound, worst error / bound = {frac:.3f}"
    assert torch.allclose(lse[fin], ref_lse[fin], rtol=2e-3, atol=1e-4), f"{what}: lse"
    return frac


def check_quantized(x, x8, descale):
    """quantize_fp8's result against the definition: the descale bit for bit, every element within one e4m3 step of the fp64
    quotient, the largest element of every head +-448."""
    x, x8, descale = x.cpu(), x8.cpu(), descale.cpu()
    amax = x.float().abs().amax(dim=(1, 3))
    want = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    assert torch.equal(descale.view(torch.int32), want.view(torch.int32)), "descale: not amax / 448 in one fp32 division"
    quo = x.double() / descale.double()[:, None, :, None]
    got = x8.double()
    step = torch.maximum(2.0 ** (torch.floor(torch.log2(quo.abs().clamp(min=2.0 ** -6))) - 3), torch.tensor(2.0 ** -9, dtype=torch.float64))
    assert torch.isfinite(got).all() and ((got - quo).abs() <= step).all(), "an element is more than one e4m3 step off x / descale"
    assert torch.equal(got.abs().amax(dim=(1, 3)), torch.where(amax > 0, 448.0, 0.0).double()), "the largest element of a head is not +-448"
