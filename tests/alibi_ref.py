"""Exact attention in fp64 with ALiBi (include/usp_hip.h: usp_flash_fwd_alibi), dense and small: the truth the ALiBi tests hold
the block kernels, the ring and the layers against.  Written on its own (plain torch on the tensors' device, one score matrix
per call); tests/test_alibi_cpu.py pins it to torch autograd of the written-out formula.

    S[i, j] = scale * q_i . k_j  -  m[b, h] * | i + off - j |,      off = Sk - Sq + shift
    row i sees key j  iff  i + off - left <= j <= i + off + right   (the mask, applied after the bias)

a negative bound is unbounded on that side, `causal` sets right = 0; GQA: query head h reads KV head h // (Hq / Hkv); `slopes`
is (Hq,) or (B, Hq) (None: no bias); rows without a visible key give lse = -inf, out = 0, dq = 0.  `lse` is the true logsumexp of
the biased scores.  The bias is additive: dS, dQ, dK, dV are formed as without it from P = exp(S - lse); the slopes get no gradient.
With shift = 0 and the unsharded tensors this is ALiBi over the GLOBAL positions of a ring.
"""
import torch

from shift_ref import visible


def default_slopes(H, device=None):
    """2^(-8 (h + 1) / H), fp32 (the ALiBi paper's geometric sequence for a power-of-two head count)."""
    return torch.tensor([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], dtype=torch.float32, device=device)


def bias(slopes, B, Hq, Sq, Sk, shift=0, device=None):
    """(B, Hq, Sq, Sk) fp64: -m[b, h] * |i + (Sk - Sq + shift) - j|; zeros for slopes = None."""
    if slopes is None:
        return torch.zeros(B, Hq, Sq, Sk, dtype=torch.float64, device=device)
    m = slopes.to(device=device, dtype=torch.float64)
    m = m[None, :].expand(B, Hq) if m.dim() == 1 else m
    assert tuple(m.shape) == (B, Hq), (tuple(m.shape), B, Hq)
    i = torch.arange(Sq, device=device)[:, None] + (Sk - Sq + int(shift))
    j = torch.arange(Sk, device=device)[None, :]
    return -m[:, :, None, None] * (i - j).abs().to(torch.float64)[None, None]


def _scores(q, k, scale, slopes, causal, window, shift):
    """q (B,Sq,Hq,D), k (B,Sk,Hkv,D) -> (masked biased scores (B,Hq,Sq,Sk) fp64, k repeated to Hq heads)."""
    B, Sq, Hq, _ = q.shape
    Sk = k.shape[1]
    k64 = k.to(torch.float64).repeat_interleave(Hq // k.shape[2], dim=2)
    s = torch.einsum("bihd,bjhd->bhij", q.to(torch.float64), k64) * scale + bias(slopes, B, Hq, Sq, Sk, shift, q.device)
    return s.masked_fill(~visible(Sq, Sk, causal, window, shift, q.device), float("-inf")), k64


def _probs(s, lse):
    fin = torch.isfinite(lse)
    return torch.where(fin[..., None], torch.exp(s - torch.where(fin, lse, torch.zeros_like(lse))[..., None]), torch.zeros_like(s))


def ref_fwd(q, k, v, scale, slopes=None, causal=False, window=None, shift=0):
    """-> (out (B,Sq,Hq,D), lse (B,Hq,Sq)), fp64 on q's device."""
    s, _ = _scores(q, k, scale, slopes, causal, window, shift)
    lse = torch.logsumexp(s, dim=-1)                                   # -inf for a row without a visible key
    v64 = v.to(torch.float64).repeat_interleave(q.shape[2] // v.shape[2], dim=2)
    return torch.einsum("bhij,bjhd->bihd", _probs(s, lse), v64), lse


def ref_bwd_from(dout, q, k, v, out, lse, scale, slopes=None, causal=False, window=None, shift=0):
    """Block backward given the rows' lse (B,Hq,Sq) and out (delta = rowsum(dout * out)) -> (dq, dk, dv), fp64.  (lse / out may be
    the GLOBAL rows' values while q x k is one block of a ring: P = exp(S - lse) is then the block's share.)"""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    s, k64 = _scores(q, k, scale, slopes, causal, window, shift)
    p = _probs(s, lse.to(torch.float64))
    do64, q64 = dout.to(torch.float64), q.to(torch.float64)
    v64 = v.to(torch.float64).repeat_interleave(G, dim=2)
    delta = (do64 * out.to(torch.float64)).sum(-1).transpose(1, 2)     # (B,Hq,Sq)
    ds = p * (torch.einsum("bihd,bjhd->bhij", do64, v64) - delta[..., None]) * scale
    dq = torch.einsum("bhij,bjhd->bihd", ds, k64)
    dk = torch.einsum("bhij,bihd->bjhd", ds, q64).reshape(B, Sk, Hkv, G, D).sum(3)
    dv = torch.einsum("bhij,bihd->bjhd", p, do64).reshape(B, Sk, Hkv, G, D).sum(3)
    return dq, dk, dv


def ref_bwd(dout, q, k, v, scale, slopes=None, causal=False, window=None, shift=0, out_dtype=None):
    """Forward + backward of the whole problem -> (out, lse, dq, dk, dv), fp64.  `out_dtype`: round `out` to it before delta is
    formed (what a 16-bit kernel's backward reads)."""
    out, lse = ref_fwd(q, k, v, scale, slopes, causal, window, shift)
    o = out if out_dtype is None else out.to(out_dtype)
    return (out, lse) + ref_bwd_from(dout, q, k, v, o, lse, scale, slopes, causal, window, shift)
