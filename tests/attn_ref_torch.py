"""Exact attention in fp64, written in plain torch so that the same code runs on the CPU (small shapes, checked against
the numpy oracle) and on the GPU (every element of a launch of 1e9 - 1e11 scores, where the numpy oracle would take
minutes).  Semantics are the library's (include/usp_hip.h) and the oracle's (oracle/usp_oracle.py):

- GQA: query head h reads KV head h // (Hq / Hkv);
- causal masks are bottom-right aligned (key j visible to row i iff j <= i + Sk - Sq);
- `window` = flash-attn's window_size (left, right): i + Sk - Sq - left <= j <= i + Sk - Sq + right, a negative bound
  is unbounded on that side, causal sets right = 0;
- `softcap` = cap: S' = cap * tanh(S * scale / cap) before the mask (None / 0 = off);
- rows without a visible key give lse = -inf, out = 0, dq = 0.

Query rows are processed in chunks whose score matrix stays below `chunk_bytes`; each chunk reads only the key range its
rows can see, so a causal launch costs half the scores of a full one.  The backward follows the block contract of
O.block_bwd and the fuzz tests: it takes the exact lse and the 16-bit-rounded out (delta = rowsum(dout * out16)).
"""
import torch

CHUNK_BYTES = 256 << 20


def _bounds(Sq, Sk, causal, window):
    left, right = (-1, -1) if window is None else (int(window[0]), int(window[1]))
    if causal:
        right = 0
    return left, right, Sk - Sq


def _key_range(r0, r1, Sk, left, right, off):
    """[k0, k1) = the keys any of the rows [r0, r1) can see."""
    k1 = Sk if right < 0 else max(0, min(Sk, r1 - 1 + off + right + 1))
    k0 = 0 if left < 0 else max(0, min(Sk, r0 + off - left))
    return k0, max(k0, k1)


def _chunks(Sq, Sk, Hq, left, right, off, chunk_bytes):
    """(r0, r1, k0, k1) with Hq * (r1 - r0) * (k1 - k0) * 8 <= chunk_bytes (at least one row)."""
    budget = max(1, chunk_bytes // (8 * Hq))
    r0 = 0
    while r0 < Sq:
        rows = max(1, budget // max(1, Sk))
        while r0 + 2 * rows <= Sq:
            k0, k1 = _key_range(r0, r0 + 2 * rows, Sk, left, right, off)
            if 2 * rows * (k1 - k0) > budget:
                break
            rows *= 2
        r1 = min(Sq, r0 + rows)
        yield (r0, r1) + _key_range(r0, r1, Sk, left, right, off)
        r0 = r1


def _scores(qc, kc, r0, k0, scale, softcap, left, right, off):
    """qc (Hkv, G, rows, D), kc (Hkv, ks, D) fp64 -> (masked S' (Hkv, G, rows, ks), tanh term or None, visibility)."""
    s = torch.matmul(qc, kc.unsqueeze(1).transpose(-1, -2)) * scale
    t = None
    if softcap:
        t = torch.tanh(s / softcap)
        s = softcap * t
    dev = qc.device
    i = torch.arange(r0, r0 + qc.shape[2], device=dev)[:, None] + off
    j = torch.arange(k0, k0 + kc.shape[1], device=dev)[None, :]
    vis = torch.ones(i.shape[0], j.shape[1], dtype=torch.bool, device=dev)
    if right >= 0:
        vis &= j <= i + right
    if left >= 0:
        vis &= j >= i - left
    return s.masked_fill(~vis, float("-inf")), t, vis


def _heads(x, r0, r1, Hkv):
    """(rows, Hq, D) slice -> (Hkv, G, rows, D) fp64."""
    rows, Hq, D = x[r0:r1].shape
    return x[r0:r1].to(torch.float64).reshape(rows, Hkv, Hq // Hkv, D).permute(1, 2, 0, 3)


def _unheads(y):
    """(Hkv, G, rows, D) -> (rows, Hq, D)."""
    Hkv, G, rows, D = y.shape
    return y.permute(2, 0, 1, 3).reshape(rows, Hkv * G, D)


def ref_fwd(q, k, v, scale, causal=False, window=None, softcap=None, chunk_bytes=CHUNK_BYTES):
    """q (B,Sq,Hq,D), k / v (B,Sk,Hkv,D), any float dtype -> (out (B,Sq,Hq,D), lse (B,Hq,Sq)) in fp64 on q's device."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    left, right, off = _bounds(Sq, Sk, causal, window)
    out = torch.zeros((B, Sq, Hq, D), dtype=torch.float64, device=q.device)
    lse = torch.full((B, Hq, Sq), float("-inf"), dtype=torch.float64, device=q.device)
    for b in range(B):
        for r0, r1, k0, k1 in _chunks(Sq, Sk, Hq, left, right, off, chunk_bytes):
            if k1 <= k0:
                continue                                   # no visible key: out 0, lse -inf
            kc, vc = (x[b, k0:k1].to(torch.float64).permute(1, 0, 2) for x in (k, v))
            s, _, _ = _scores(_heads(q[b], r0, r1, Hkv), kc, r0, k0, scale, softcap, left, right, off)
            m = s.amax(-1, keepdim=True)
            m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
            p = torch.exp(s - m)
            l = p.sum(-1, keepdim=True)
            lse[b, :, r0:r1] = (m + torch.log(l))[..., 0].reshape(Hq, r1 - r0)
            att = torch.where(l > 0, p / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(p))
            out[b, r0:r1] = _unheads(torch.matmul(att, vc.unsqueeze(1)))
    return out, lse


def ref_delta(dout, out16):
    """delta (B,Hq,Sq) fp64 = rowsum(dout * out16): the backward's D term from the 16-bit-rounded out."""
    return (dout.to(torch.float64) * out16.to(torch.float64)).sum(-1).transpose(1, 2).contiguous()


def ref_bwd(dout, q, k, v, out16, lse, scale, causal=False, window=None, softcap=None, chunk_bytes=CHUNK_BYTES):
    """Block backward given the exact lse (B,Hq,Sq) and the 16-bit out -> (dq, dk, dv, delta), fp64 on q's device."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    left, right, off = _bounds(Sq, Sk, causal, window)
    delta = ref_delta(dout, out16)
    lse = lse.to(device=q.device, dtype=torch.float64)
    dq = torch.zeros((B, Sq, Hq, D), dtype=torch.float64, device=q.device)
    dk = torch.zeros((B, Sk, Hkv, D), dtype=torch.float64, device=q.device)
    dv = torch.zeros_like(dk)
    for b in range(B):
        for r0, r1, k0, k1 in _chunks(Sq, Sk, Hq, left, right, off, chunk_bytes):
            if k1 <= k0:
                continue
            rows = r1 - r0
            qc, doc = _heads(q[b], r0, r1, Hkv), _heads(dout[b], r0, r1, Hkv)
            kc, vc = (x[b, k0:k1].to(torch.float64).permute(1, 0, 2) for x in (k, v))
            s, t, _ = _scores(qc, kc, r0, k0, scale, softcap, left, right, off)
            l = lse[b, :, r0:r1].reshape(Hkv, G, rows, 1)
            fin = torch.isfinite(l)
            p = torch.where(fin, torch.exp(s - torch.where(fin, l, torch.zeros_like(l))), torch.zeros_like(s))
            dl = delta[b, :, r0:r1].reshape(Hkv, G, rows, 1)
            dv[b, k0:k1] += torch.matmul(p.transpose(-1, -2), doc).sum(1).permute(1, 0, 2)
            ds = p * (torch.matmul(doc, vc.unsqueeze(1).transpose(-1, -2)) - dl)
            if softcap:
                ds = ds * (1.0 - t * t)
            ds = ds * scale
            dq[b, r0:r1] = _unheads(torch.matmul(ds, kc.unsqueeze(1)))
            dk[b, k0:k1] += torch.matmul(ds.transpose(-1, -2), qc).sum(1).permute(1, 0, 2)
    return dq, dk, dv, delta
