"""Exact attention in fp64 under an interval mask -- row i sees key j iff row_lo[i] <= j < row_hi[i] -- in the style of
tests/attn_ref_torch.py: plain torch on the tensors' device, query rows in chunks whose score matrix stays below `chunk_bytes`,
each chunk reading only the keys [min row_lo, max row_hi) of its rows that see anything.  It is what tests/span_ref.py,
tests/doc_ref.py and tests/sink_ref.py compute with one dense score matrix per call (tests/test_large_launch_masks_cpu.py pins it
to them at 1e-10), at the sizes of tests/test_gpu_large_launch_masks.py, where a dense matrix does not fit.

- `row_lo`, `row_hi`: (B, Sq) or (Sq,) integers (numpy or torch), in the launch's own key numbering; they need not be monotone;
- GQA: query head h reads KV head h // (Hq / Hkv);
- `sinks` (Hq,), in score units: the logit of head h joins every row's denominator and `lse` and carries no value;
- rows that see nothing give out = 0, lse = -inf, dq = 0; with a sink lse = s_h.

The bounds themselves come from the GLOBAL definition (tests/span_ref.py: global_mask), never from the planner: `bounds` below
computes start(i) and hi(i) over the whole sequence as global_mask does and, for a ring block, slices and rebases them.
"""
import numpy as np
import torch

from attn_ref_torch import CHUNK_BYTES, _heads, _unheads, ref_delta


# ---- the bounds, from the global definition ----------------------------------------------------------------------------------
def bounds(S_total, cu=None, spans=(), row0=0, Sq=None, key0=0, Sk=None):
    """(row_lo, row_hi) int64 (Sq,) of the launch whose rows are the global positions [row0, row0 + Sq) and whose keys are
    [key0, key0 + Sk) (default: the whole sequence), for ONE list of cumulative document lengths `cu` (None: one document) and its
    `spans`: global row i sees global key j iff start(i) <= j < hi(i), start(i) the first position of the document that holds i,
    hi(i) the end of the span that holds i, i + 1 where none does.  The causal diagonal is hi's `i + 1`: for the whole sequence
    row_hi = i + 1, for a block i + 1 + (row0 - key0), clamped to the block's keys like every bound."""
    Sq = S_total if Sq is None else Sq
    Sk = S_total if Sk is None else Sk
    start = np.zeros(S_total, dtype=np.int64)
    for s, e in zip((cu or [0, S_total])[:-1], (cu or [0, S_total])[1:]):
        start[s:e] = s
    hi = np.arange(S_total, dtype=np.int64) + 1
    for s, e in spans:
        hi[s:e] = e
    rows = slice(row0, row0 + Sq)
    return np.clip(start[rows] - key0, 0, Sk), np.clip(hi[rows] - key0, 0, Sk)


def window_bounds(Sq, Sk, causal=True, window=None):
    """(row_lo, row_hi) int64 (Sq,) of a causal and / or windowed launch (include/usp_hip.h): row i sees key j iff
    i + (Sk - Sq) - left <= j <= i + (Sk - Sq) + right, a negative bound unbounded, `causal` sets right = 0."""
    left, right = (-1, -1) if window is None else (int(window[0]), int(window[1]))
    if causal:
        right = 0
    d = np.arange(Sq, dtype=np.int64) + (Sk - Sq)
    lo = np.zeros(Sq, dtype=np.int64) if left < 0 else np.clip(d - left, 0, Sk)
    hi = np.full(Sq, Sk, dtype=np.int64) if right < 0 else np.clip(d + right + 1, 0, Sk)
    return lo, hi


def key_bounds(row_lo, row_hi, Sk):
    """(key_lo, key_hi) int64 (Sk,) of MONOTONE row bounds (asserted): key j is seen by the rows key_lo[j] <= i < key_hi[j], the
    leading rows with row_lo <= j less the leading ones with row_hi <= j."""
    lo, hi = np.asarray(row_lo, dtype=np.int64), np.asarray(row_hi, dtype=np.int64)
    assert (np.diff(lo) >= 0).all() and (np.diff(hi) >= 0).all(), "key_bounds needs non-decreasing row bounds"
    keys = np.arange(Sk, dtype=np.int64)
    return np.searchsorted(hi, keys, side="right"), np.searchsorted(lo, keys, side="right")


# ---- the reference -----------------------------------------------------------------------------------------------------------
def _per_batch(x, B, Sq):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    a = a.astype(np.int64).reshape(-1, Sq)
    assert a.shape[0] in (1, B), (a.shape, B)
    return np.broadcast_to(a, (B, Sq))


def _key_range(lo, hi, r0, r1):
    """[k0, k1) = the keys any of the rows [r0, r1) sees; (0, 0) when none sees a key."""
    a, b = lo[r0:r1], hi[r0:r1]
    sees = a < b
    if not sees.any():
        return 0, 0
    return int(a[sees].min()), int(b[sees].max())


def _chunks(lo, hi, Hq, chunk_bytes):
    """(r0, r1, k0, k1) with Hq * (r1 - r0) * (k1 - k0) * 8 <= chunk_bytes (at least one row), covering every row once."""
    Sq = len(lo)
    budget = max(1, chunk_bytes // (8 * Hq))
    r0 = 0
    while r0 < Sq:
        rows = 1
        while r0 + rows < Sq:
            nxt = min(2 * rows, Sq - r0)
            k0, k1 = _key_range(lo, hi, r0, r0 + nxt)
            if nxt * (k1 - k0) > budget:
                break
            rows = nxt
        yield (r0, r0 + rows) + _key_range(lo, hi, r0, r0 + rows)
        r0 += rows


def _scores(qc, kc, lo, hi, r0, r1, k0, scale):
    """qc (Hkv, G, rows, D), kc (Hkv, ks, D) fp64 -> S masked to -inf outside [lo, hi) (Hkv, G, rows, ks)."""
    dev = qc.device
    s = torch.matmul(qc, kc.unsqueeze(1).transpose(-1, -2)) * scale
    j = torch.arange(k0, k0 + kc.shape[1], device=dev)[None, :]
    a = torch.from_numpy(np.array(lo[r0:r1])).to(dev)[:, None]
    b = torch.from_numpy(np.array(hi[r0:r1])).to(dev)[:, None]
    return s.masked_fill(~((j >= a) & (j < b)), float("-inf"))


def ref_fwd(q, k, v, scale, row_lo, row_hi, sinks=None, chunk_bytes=CHUNK_BYTES):
    """q (B,Sq,Hq,D), k / v (B,Sk,Hkv,D), any float dtype -> (out (B,Sq,Hq,D), lse (B,Hq,Sq)) in fp64 on q's device."""
    B, Sq, Hq, D = q.shape
    Hkv = k.shape[2]
    G = Hq // Hkv
    los, his = _per_batch(row_lo, B, Sq), _per_batch(row_hi, B, Sq)
    out = torch.zeros((B, Sq, Hq, D), dtype=torch.float64, device=q.device)
    lse = torch.full((B, Hq, Sq), float("-inf"), dtype=torch.float64, device=q.device)
    sk = None if sinks is None else sinks.detach().to(device=q.device, dtype=torch.float64)
    if sk is not None:
        lse[:] = sk[None, :, None]                         # a row that sees nothing: lse = s_h, out = 0
    for b in range(B):
        for r0, r1, k0, k1 in _chunks(los[b], his[b], Hq, chunk_bytes):
            if k1 <= k0:
                continue
            kc, vc = (x[b, k0:k1].to(torch.float64).permute(1, 0, 2) for x in (k, v))
            s = _scores(_heads(q[b], r0, r1, Hkv), kc, los[b], his[b], r0, r1, k0, scale)
            m = s.amax(-1, keepdim=True)
            if sk is not None:
                m = torch.maximum(m, sk.reshape(Hkv, G, 1, 1))
            m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
            p = torch.exp(s - m)
            l = p.sum(-1, keepdim=True)
            if sk is not None:
                l = l + torch.exp(sk.reshape(Hkv, G, 1, 1) - m)
            lse[b, :, r0:r1] = (m + torch.log(l))[..., 0].reshape(Hq, r1 - r0)
            att = torch.where(l > 0, p / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(p))
            out[b, r0:r1] = _unheads(torch.matmul(att, vc.unsqueeze(1)))
    return out, lse


def ref_bwd(dout, q, k, v, out16, lse, scale, row_lo, row_hi, chunk_bytes=CHUNK_BYTES):
    """Block backward given the exact (sink-including) lse (B,Hq,Sq) and the 16-bit out -> (dq, dk, dv, delta), fp64 on q's
    device: P = exp(S - lse), dS = P (dout v^T - delta) scale, delta = rowsum(dout * out16)."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    los, his = _per_batch(row_lo, B, Sq), _per_batch(row_hi, B, Sq)
    delta = ref_delta(dout, out16)
    lse = lse.to(device=q.device, dtype=torch.float64)
    dq = torch.zeros((B, Sq, Hq, D), dtype=torch.float64, device=q.device)
    dk = torch.zeros((B, Sk, Hkv, D), dtype=torch.float64, device=q.device)
    dv = torch.zeros_like(dk)
    for b in range(B):
        for r0, r1, k0, k1 in _chunks(los[b], his[b], Hq, chunk_bytes):
            if k1 <= k0:
                continue
            rows = r1 - r0
            qc, doc = _heads(q[b], r0, r1, Hkv), _heads(dout[b], r0, r1, Hkv)
            kc, vc = (x[b, k0:k1].to(torch.float64).permute(1, 0, 2) for x in (k, v))
            s = _scores(qc, kc, los[b], his[b], r0, r1, k0, scale)
            l = lse[b, :, r0:r1].reshape(Hkv, G, rows, 1)
            fin = torch.isfinite(l)
            p = torch.where(fin, torch.exp(s - torch.where(fin, l, torch.zeros_like(l))), torch.zeros_like(s))
            dl = delta[b, :, r0:r1].reshape(Hkv, G, rows, 1)
            dv[b, k0:k1] += torch.matmul(p.transpose(-1, -2), doc).sum(1).permute(1, 0, 2)
            ds = p * (torch.matmul(doc, vc.unsqueeze(1).transpose(-1, -2)) - dl) * scale
            dq[b, r0:r1] = _unheads(torch.matmul(ds, kc.unsqueeze(1)))
            dk[b, k0:k1] += torch.matmul(ds.transpose(-1, -2), qc).sum(1).permute(1, 0, 2)
    return dq, dk, dv, delta
