"""Exact attention in fp64 with dropout (include/usp_hip.h: usp_flash_fwd_dropout), dense and small: the truth the dropout tests
hold the block kernels, the ring and the layers against.  Written from the header's text on its own (numpy integers for the
generator, plain torch for the attention); it shares no code with csrc/usp_dropout_rng.h, and tests/test_dropout_cpu.py pins it to
the Random123 known answers, to that header, and to torch autograd of the written-out formula.

    t          = min(256, max(1, rint((1 - p) * 256)))   in float32, ties to even
    w[4]       = Philox4x32-10(counter = (i >> 2, j >> 2, h, b), key = (seed & 0xffffffff, seed >> 32))
    keep(i, j) = ((w[i & 3] >> (8 * (j & 3))) & 0xff) < t        i, j, h: GLOBAL row, key, QUERY head (row0 / key0 / head0 + local)
    P = softmax of the masked scores;  lse = logsumexp (un-dropped);  out = (256 / t) (keep o P) V
    delta = rowsum(dout * out);  dV = (256 / t) (keep o P)^T dO;  dS = P ((256 / t) keep (dO V^T) - delta) scale;  dQ = dS K;  dK = dS^T Q

The mask (causal / window / shift) is tests/shift_ref.py's `visible`; GQA: query head h reads KV head h // (Hq / Hkv); rows
without a visible key give lse = -inf, out = 0 and zero gradients.
"""
import numpy as np
import torch

from shift_ref import visible

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def threshold(p):
    """Keep threshold of drop probability p, formed in float32 as the library does."""
    t = int(np.rint((np.float32(1.0) - np.float32(p)) * np.float32(256.0)))
    return min(256, max(1, t))


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on broadcastable integer arrays -> four uint64 arrays holding 32-bit words."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK32) for x in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]                    # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c


_BYTES = {}          # the last few windows of keep_bytes (read-only arrays): the bytes do not depend on p, dtype or head dim


def keep_bytes(seed, B, H, rows, keys, row0=0, key0=0, head0=0):
    """(B, H, rows, keys) uint8: the byte compared with the threshold for every (batch, head, row, key).  One Philox call per
    4 x 4 patch, as the definition has it; the patches that the window touches are expanded and cut to it."""
    key = (int(seed), B, H, rows, keys, int(row0), int(key0), int(head0))
    if key not in _BYTES:
        while len(_BYTES) >= 4:
            _BYTES.pop(next(iter(_BYTES)))
        _BYTES[key] = _keep_bytes(*key)
        _BYTES[key].setflags(write=False)
    return _BYTES[key]


def _keep_bytes(seed, B, H, rows, keys, row0, key0, head0):
    seed, row0, key0 = int(seed), int(row0), int(key0)
    pr0, pr1 = row0 >> 2, (row0 + rows - 1) >> 2
    pk0, pk1 = key0 >> 2, (key0 + keys - 1) >> 2
    pi = np.arange(pr0, pr1 + 1, dtype=np.uint64)[None, None, :, None]
    pj = np.arange(pk0, pk1 + 1, dtype=np.uint64)[None, None, None, :]
    h = (np.arange(H, dtype=np.uint64) + np.uint64(head0))[None, :, None, None]
    b = np.arange(B, dtype=np.uint64)[:, None, None, None]
    w = np.stack(philox4x32_10(pi, pj, h, b, seed & MASK32, seed >> 32), axis=3)          # (B, H, patch rows, 4 words, patch keys)
    shifts = (np.uint64(8) * np.arange(4, dtype=np.uint64))
    by = ((w[..., None] >> shifts) & np.uint64(0xFF)).astype(np.uint8)                    # (..., 4 rows, patch keys, 4 keys)
    full = by.reshape(B, H, 4 * (pr1 - pr0 + 1), 4 * (pk1 - pk0 + 1))
    r0, c0 = row0 - 4 * pr0, key0 - 4 * pk0
    return np.ascontiguousarray(full[:, :, r0:r0 + rows, c0:c0 + keys])


def keep_mask(p, seed, B, H, rows, keys, row0=0, key0=0, head0=0):
    """(B, H, rows, keys) bool numpy array: True where the probability is kept."""
    return keep_bytes(seed, B, H, rows, keys, row0, key0, head0).astype(np.int32) < threshold(p)


def rescale(p):
    return 256.0 / threshold(p)


def _keep(p, seed, B, Hq, Sq, Sk, at, device):
    """(keep (B,Hq,Sq,Sk) fp64, 256/t); at = (row0, key0, head0).  p = 0 / None: all ones."""
    if not p:
        return torch.ones(B, Hq, Sq, Sk, dtype=torch.float64, device=device), 1.0
    if threshold(p) == 256:
        return torch.ones(B, Hq, Sq, Sk, dtype=torch.float64, device=device), 1.0
    m = keep_mask(p, seed, B, Hq, Sq, Sk, *at)
    return torch.from_numpy(m).to(device).to(torch.float64), rescale(p)       # (converted on the device)


def _scores(q, k, scale, causal, window, shift):
    B, Sq, Hq, _ = q.shape
    Sk = k.shape[1]
    k64 = k.to(torch.float64).repeat_interleave(Hq // k.shape[2], dim=2)
    s = torch.einsum("bihd,bjhd->bhij", q.to(torch.float64), k64) * scale
    return s.masked_fill(~visible(Sq, Sk, causal, window, shift, q.device), float("-inf")), k64


def _probs(s, lse):
    fin = torch.isfinite(lse)
    return torch.where(fin[..., None], torch.exp(s - torch.where(fin, lse, torch.zeros_like(lse))[..., None]), torch.zeros_like(s))


def ref_fwd(q, k, v, scale, p=0.0, seed=0, at=(0, 0, 0), causal=False, window=None, shift=0, keep=None):
    """-> (out (B,Sq,Hq,D), lse (B,Hq,Sq)), fp64 on q's device.  `keep` = (mask, factor) overrides the generator (mutants)."""
    B, Sq, Hq, _ = q.shape
    s, _ = _scores(q, k, scale, causal, window, shift)
    lse = torch.logsumexp(s, dim=-1)
    kp, rs = keep if keep is not None else _keep(p, seed, B, Hq, Sq, k.shape[1], at, q.device)
    v64 = v.to(torch.float64).repeat_interleave(Hq // v.shape[2], dim=2)
    return rs * torch.einsum("bhij,bjhd->bihd", _probs(s, lse) * kp, v64), lse


def ref_bwd_from(dout, q, k, v, out, lse, scale, p=0.0, seed=0, at=(0, 0, 0), causal=False, window=None, shift=0, keep=None):
    """Block backward given the rows' lse (B,Hq,Sq) and the dropped out (delta = rowsum(dout * out)) -> (dq, dk, dv), fp64."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    s, k64 = _scores(q, k, scale, causal, window, shift)
    pr = _probs(s, lse.to(torch.float64))
    kp, rs = keep if keep is not None else _keep(p, seed, B, Hq, Sq, Sk, at, q.device)
    do64, q64 = dout.to(torch.float64), q.to(torch.float64)
    v64 = v.to(torch.float64).repeat_interleave(G, dim=2)
    delta = (do64 * out.to(torch.float64)).sum(-1).transpose(1, 2)     # (B,Hq,Sq)
    ds = pr * (rs * kp * torch.einsum("bihd,bjhd->bhij", do64, v64) - delta[..., None]) * scale
    dq = torch.einsum("bhij,bjhd->bihd", ds, k64)
    dk = torch.einsum("bhij,bihd->bjhd", ds, q64).reshape(B, Sk, Hkv, G, D).sum(3)
    dv = rs * torch.einsum("bhij,bihd->bjhd", pr * kp, do64).reshape(B, Sk, Hkv, G, D).sum(3)
    return dq, dk, dv


def ref_bwd(dout, q, k, v, scale, p=0.0, seed=0, at=(0, 0, 0), causal=False, window=None, shift=0, out_dtype=None, keep=None):
    """Forward + backward of the whole problem -> (out, lse, dq, dk, dv), fp64.  `out_dtype`: round `out` to it before delta is
    formed (what a 16-bit kernel's backward reads)."""
    out, lse = ref_fwd(q, k, v, scale, p, seed, at, causal, window, shift, keep)
    o = out if out_dtype is None else out.to(out_dtype)
    return (out, lse) + ref_bwd_from(dout, q, k, v, o, lse, scale, p, seed, at, causal, window, shift, keep)
