"""Exact attention in fp64 with a SHIFTED mask diagonal (include/usp_hip.h, USP_ATTN_SHIFT), dense and small: the truth the
windowed-ring tests hold the block kernels, the planner's blocks and the ring against.  Written on its own (plain torch, one
score matrix per call); tests/test_ring_window_cpu.py pins it to tests/attn_ref_torch.py at shift = 0.

    row i sees key j  iff  i + off - left <= j <= i + off + right,   off = Sk - Sq + shift

a negative bound is unbounded on that side, `causal` sets right = 0; GQA: query head h reads KV head h // (Hq / Hkv);
softcap: S' = cap * tanh(S * scale / cap) before the mask; rows without a visible key give lse = -inf, out = 0, dq = 0.
With shift = 0 and the unsharded tensors this is the GLOBAL window of ring/window_blocks.py.
"""
import torch


def visible(Sq, Sk, causal=False, window=None, shift=0, device=None):
    """(Sq, Sk) bool."""
    left, right = (-1, -1) if window is None else (int(window[0]), int(window[1]))
    if causal:
        right = 0
    i = torch.arange(Sq, device=device)[:, None] + (Sk - Sq + int(shift))
    j = torch.arange(Sk, device=device)[None, :]
    vis = torch.ones(Sq, Sk, dtype=torch.bool, device=device)
    if right >= 0:
        vis &= j <= i + right
    if left >= 0:
        vis &= j >= i - left
    return vis


def _scores(q, k, scale, causal, window, shift, softcap):
    """q (B,Sq,Hq,D), k (B,Sk,Hkv,D) -> (masked S' (B,Hq,Sq,Sk) fp64, tanh term | None, k repeated to Hq heads)."""
    G = q.shape[2] // k.shape[2]
    q64 = q.to(torch.float64)
    k64 = k.to(torch.float64).repeat_interleave(G, dim=2)
    s = torch.einsum("bihd,bjhd->bhij", q64, k64) * scale
    t = None
    if softcap:
        t = torch.tanh(s / softcap)
        s = softcap * t
    vis = visible(q.shape[1], k.shape[1], causal, window, shift, q.device)
    return s.masked_fill(~vis, float("-inf")), t, k64


def ref_fwd(q, k, v, scale, causal=False, window=None, shift=0, softcap=None):
    """-> (out (B,Sq,Hq,D), lse (B,Hq,Sq)), fp64 on q's device."""
    s, _, _ = _scores(q, k, scale, causal, window, shift, softcap)
    lse = torch.logsumexp(s, dim=-1)                                   # -inf for a row without a visible key
    fin = torch.isfinite(lse)
    p = torch.where(fin[..., None], torch.exp(s - torch.where(fin, lse, torch.zeros_like(lse))[..., None]), torch.zeros_like(s))
    v64 = v.to(torch.float64).repeat_interleave(q.shape[2] // v.shape[2], dim=2)
    return torch.einsum("bhij,bjhd->bihd", p, v64), lse


def ref_bwd(dout, q, k, v, out, lse, scale, causal=False, window=None, shift=0, softcap=None):
    """Block backward given the rows' lse (B,Hq,Sq) and out (delta = rowsum(dout * out)) -> (dq, dk, dv), fp64."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    s, t, k64 = _scores(q, k, scale, causal, window, shift, softcap)
    lse = lse.to(torch.float64)
    fin = torch.isfinite(lse)
    p = torch.where(fin[..., None], torch.exp(s - torch.where(fin, lse, torch.zeros_like(lse))[..., None]), torch.zeros_like(s))
    do64, q64 = dout.to(torch.float64), q.to(torch.float64)
    v64 = v.to(torch.float64).repeat_interleave(G, dim=2)
    delta = (do64 * out.to(torch.float64)).sum(-1).transpose(1, 2)     # (B,Hq,Sq)
    ds = p * (torch.einsum("bihd,bjhd->bhij", do64, v64) - delta[..., None])
    if softcap:
        ds = ds * (1.0 - t * t)
    ds = ds * scale
    dq = torch.einsum("bhij,bjhd->bihd", ds, k64)
    dk = torch.einsum("bhij,bihd->bjhd", ds, q64).reshape(B, Sk, Hkv, G, D).sum(3)
    dv = torch.einsum("bhij,bihd->bjhd", p, do64).reshape(B, Sk, Hkv, G, D).sum(3)
    return dq, dk, dv
