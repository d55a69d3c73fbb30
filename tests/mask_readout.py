"""Dropout mask read-out: inputs that make the attention kernels PRINT their keep mask, and the decoder of what they print.

tests/test_gpu_dropout.py compares with tolerances; a few wrong mask bits (a ragged edge, one quad, one patch at a cut) stay
inside them.  No tolerance is needed: with q = 0 every visible score is 0, so P is 1 / N_i in the forward (N_i visible keys of
row i) and, with lse = 0 and delta = 0 GIVEN to the backward, exactly 1 there.  With "bit plane" operands -- key j (or row i)
holds the single value 2^e(j div D) in channel j mod D -- every output element is an exact integer whose bits are keep decisions:

    forward   q = 0, k = N(0,1), v = key planes                    x = acc  * N_i * t/256          bits: keep(i, d + m D)
    dQ        q = 0, k = key planes, v = e_0, dout = e_0           x = dq   / (scale * 256/t)      bits: keep(i, d + m D)
    dK        k = 0, v = e_0, dout = e_0, q = row planes           x = dk   / (scale * 256/t)      bits: keep_h(d + m D, j)
    dV        v = 0, q = 0, k = N(0,1), dout = row planes          x = dv   * t/256                bits: keep_h(d + m D, j)

(row planes carry an exponent of their own for every (query head within the KV group, i div D): the sum over the group keeps the
heads apart).  softmax_scale = 0.125, a power of two.  What does not fit one launch is read in several PASSES: each pass holds a
chunk of the planes and zeros elsewhere.  The builder asserts its conditions (they are conditions, not measurements):

  * every plane value is a normal number of the 16-bit dtype (exponents start below 0 where needed to stay under fp16's 2^15);
  * every decoded integer stays below 2^22 -- and a pass holds at most 16 planes: the MFMA accumulators hold the integer
    exactly, but the epilogues multiply it by 256/t (and by scale, 1 / N_i or a partial slab's weight) in fp32, each step a
    rounding of 2^-24 relative: four of them move x < 2^16 by at most 2^-6;
  * the dQ kernel rounds dS = 256/t to 16 bits before its MFMA (honest rounding, 2^-(mantissa bits + 1) relative): unless t is a
    power of two a dQ pass holds at most `mantissa bits - 3` planes, never more than 6 (bf16 4, fp16 6), so that the rounding
    moves x by at most 2^n 2^-(mantissa + 1) <= 1/16;
  * a pass whose result is merged by LSE weights (k_splits, merge_in) holds at most 8 planes, one decoded from the 16-bit `out`
    at most 4 (x < 16 at a relative rounding of at most 2^-8 in bf16: 1/16);

and the decoder requires |x - rint(x)| < 1/8 of every element.  Plain numpy and torch; runs anywhere.
"""
import collections
import math

import numpy as np
import torch

import dropout_ref
from shift_ref import visible

SCALE = 0.125
PROBS = {1.0 / 256: 255, 0.1: 230, 0.5: 128, 0.75: 64, 0.9: 26, 255.0 / 256: 1}       # p -> keep threshold t
INT_BITS, PASS_PLANES, MERGED_PLANES, OUT16_PLANES, MAX_DEV = 22, 16, 8, 4, 0.125
KINDS = ("fwd", "dq", "dk", "dv")

Shape = collections.namedtuple("Shape", "B Sq Sk Hq Hkv D dt")
Pass = collections.namedtuple("Pass", "q k v dout planes lo")      # planes: key planes m, or row planes (g, m); lo: exponent of bit 0


def _exponents(dt):
    """(mantissa bits, smallest normal exponent, largest exponent used): plane values stay below 2^15 in either dtype."""
    fi = torch.finfo(getattr(torch, dt))
    return int(round(-math.log2(fi.eps))), int(round(math.log2(fi.tiny))), 14


def plane_cap(kind, dt, p, merged=False, out16=False):
    """Planes one pass may hold (module docstring)."""
    mant, emin, emax = _exponents(dt)
    cap = min(INT_BITS, PASS_PLANES, emax - emin + 1)
    t = dropout_ref.threshold(p)
    if kind == "dq" and t & (t - 1):
        cap = min(cap, 6, mant - 3)
        assert 2.0 ** cap * 2.0 ** -(mant + 1) <= 1.0 / 16
    if merged:
        cap = min(cap, MERGED_PLANES)
    if out16:
        cap = min(cap, OUT16_PLANES)
    return cap


def all_planes(kind, s):
    if kind in ("fwd", "dq"):
        return list(range(-(-s.Sk // s.D)))
    return [(g, m) for g in range(s.Hq // s.Hkv) for m in range(-(-s.Sq // s.D))]


def _plane_tensor(kind, s, chunk, lo):
    """Key planes (B,Sk,Hkv,D) or row planes (B,Sq,Hq,D), float32."""
    if kind in ("fwd", "dq"):
        x = torch.zeros(s.Sk, s.D)
        for bit, m in enumerate(chunk):
            j = torch.arange(m * s.D, min((m + 1) * s.D, s.Sk))
            x[j, j - m * s.D] = 2.0 ** (bit + lo)
        return x[None, :, None, :].expand(s.B, s.Sk, s.Hkv, s.D).contiguous()
    G = s.Hq // s.Hkv
    x = torch.zeros(s.Sq, s.Hq, s.D)
    for bit, (g, m) in enumerate(chunk):
        i = torch.arange(m * s.D, min((m + 1) * s.D, s.Sq))
        for h in range(g, s.Hq, G):
            x[i, h, i - m * s.D] = 2.0 ** (bit + lo)
    return x[None].expand(s.B, s.Sq, s.Hq, s.D).contiguous()


def build(kind, shape, p, merged=False, out16=False, seed=0):
    """The passes of one read-out problem: [Pass(q, k, v, dout, planes, lo)], tensors of the shape's dtype on the CPU (dout is None
    in the forward).  The backward passes are to be run with lse = 0 and delta = 0."""
    s = shape
    assert kind in KINDS and s.Hq % s.Hkv == 0
    assert not (merged or out16) or kind == "fwd"
    dtype = getattr(torch, s.dt)
    mant, emin, emax = _exponents(s.dt)
    cap = plane_cap(kind, s.dt, p, merged, out16)
    planes = all_planes(kind, s)
    g = torch.Generator().manual_seed(seed)
    zq, zk = torch.zeros(s.B, s.Sq, s.Hq, s.D), torch.zeros(s.B, s.Sk, s.Hkv, s.D)
    eq, ek = zq.clone(), zk.clone()
    eq[..., 0] = 1.0
    ek[..., 0] = 1.0
    noise = torch.randn(s.B, s.Sk, s.Hkv, s.D, generator=g)
    passes = []
    for c0 in range(0, len(planes), cap):
        chunk = planes[c0:c0 + cap]
        n = len(chunk)
        lo = min(0, emax - (n - 1))
        assert n <= INT_BITS and lo >= emin, (n, lo)
        pl = _plane_tensor(kind, s, chunk, lo)
        nz = pl[pl != 0]
        assert bool((pl.to(dtype).float() == pl).all()) and float(nz.min()) >= 2.0 ** emin and float(nz.max()) <= 2.0 ** emax, \
            "every plane value is a normal number of the 16-bit dtype"
        q, k, v, do = {"fwd": (zq, noise, pl, None), "dq": (zq, pl, ek, eq), "dk": (pl, zk, ek, eq), "dv": (zq, noise, zk, pl)}[kind]
        passes.append(Pass(q.to(dtype), k.to(dtype), v.to(dtype), None if do is None else do.to(dtype), chunk, lo))
    return passes


def stats(s, device=None):
    """(lse, delta) of the backward read-outs: zeros, given as inputs."""
    return tuple(torch.zeros(s.B, s.Hq, s.Sq, dtype=torch.float32, device=device) for _ in range(2))


def _np64(t):
    return t.detach().to(torch.float64).cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def decode(kind, shape, p, passes, results, vis=None, rows=None):
    """`results`: per pass the tensor that carries the bits (fwd: acc or out (B,Sq,Hq,D); dq; dk; dv) -> (bits, largest
    |x - rint(x)|).  bits: bool (B, Hq, rows, keys), padded to whole planes (fwd / dq: keys to a multiple of D; dk / dv: rows) so
    that a bit printed for a key or row that does not exist is seen too.  `vis` (Sq, Sk) bool: the forward's N_i.  `rows`: a
    slice of the query rows to decode (fwd / dq; the others are left False)."""
    s = shape
    t = dropout_ref.threshold(p)
    G = s.Hq // s.Hkv
    Mk, Mq = -(-s.Sk // s.D), -(-s.Sq // s.D)
    key_planes = kind in ("fwd", "dq")
    bits = np.zeros((s.B, s.Hq, s.Sq, Mk * s.D) if key_planes else (s.B, s.Hq, Mq * s.D, s.Sk), dtype=bool)
    rows = slice(None) if rows is None else rows
    worst = 0.0
    assert len(passes) == len(results)
    for ps, res in zip(passes, results):
        x = _np64(res)
        if kind == "fwd":
            n_i = np.maximum(np.asarray(vis).sum(-1), 1).astype(np.float64)
            x = x * n_i[None, :, None, None] * (t / 256.0)
        elif kind == "dv":
            x = x * (t / 256.0)
        else:
            x = x / (SCALE * 256.0 / t)
        x = x * 2.0 ** -ps.lo
        if key_planes:
            x = x[:, rows]
        r = np.rint(x)
        dev = float(np.abs(x - r).max()) if x.size else 0.0
        worst = max(worst, dev)
        assert np.isfinite(x).all() and dev < MAX_DEV, f"{kind} read-out: an element lies {dev:.4f} from an integer (limit {MAX_DEV})"
        n = len(ps.planes)
        assert r.min() >= 0 and r.max() < 2.0 ** n, f"{kind} read-out: decoded integers span [{r.min():.0f}, {r.max():.0f}], {n} planes"
        r = r.astype(np.int64)
        for bit, plane in enumerate(ps.planes):
            on = ((r >> bit) & 1).astype(bool)
            if key_planes:                                   # (B, rows, Hq, D) -> [b, h, i, m D + d]
                bits[:, :, rows, plane * s.D:(plane + 1) * s.D] = on.transpose(0, 2, 1, 3)
            else:                                            # (B, Sk, Hkv, D) -> [b, hkv G + g, m D + d, j]
                g, m = plane
                bits[:, g::G, m * s.D:(m + 1) * s.D, :] = on.transpose(0, 2, 3, 1)
    return bits, worst


def expected(shape, p, seed, at=(0, 0, 0), causal=False, window=None, shift=0):
    """"Visible and kept": bool numpy (B, Hq, Sq, Sk)."""
    s = shape
    vis = visible(s.Sq, s.Sk, causal, window, shift).numpy()
    return dropout_ref.keep_mask(p, seed, s.B, s.Hq, s.Sq, s.Sk, *at) & vis[None, None]


def wrong_bits(bits, want):
    """Positions (N, 4) = (batch, head, local row, local key) where the decoded bits (possibly padded) differ from `want`."""
    full = np.zeros(bits.shape, dtype=bool)
    full[:, :, :want.shape[2], :want.shape[3]] = want
    return np.argwhere(bits != full)


def report(bad, at=(0, 0, 0)):
    """The decoder's failure text: how many bits, the first ten as (batch, head, GLOBAL row, GLOBAL key), and for each the key
    tile (key // 64), row mod 32 and key mod 4 of the launch: the lane group names itself."""
    lines = [f"{len(bad)} wrong mask bits; (batch, head, global row, global key) [key tile, row mod 32, key mod 4]:"]
    for b, h, i, j in bad[:10]:
        lines.append(f"  ({b}, {h + at[2]}, {i + at[0]}, {j + at[1]}) [tile {j // 64}, row%32 {i % 32}, key%4 {j % 4}]")
    return "\n".join(lines)


def compare(bits, want, at=(0, 0, 0), what=""):
    """Fails with `report` unless the decoded bits equal `want`; returns the number of bits compared."""
    bad = wrong_bits(bits, want)
    assert len(bad) == 0, f"{what}: {report(bad, at)}"
    return int(want.size)
