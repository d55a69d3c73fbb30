#!/usr/bin/env python3
"""Rates of the gathered-key forward (key_index=) beside the dense causal forward and the block_mask forward on the 128-block cover
of the same pattern, on one GPU (-> profiles/key_index_rates.txt).

    python tools/key_index_rates.py [--rounds 15] [--reps 5] [--seq 32768] [--left 1023] [--n 1024] [--bwd]

Case: B1 H32/4 D128 bf16 causal, a band of `left` keys below the diagonal plus `n` listed keys per head drawn uniformly from the
sequence.  Device events around `reps` launches, warm-up first, medians of `rounds` rounds with the variants interleaved inside each
round; the spread of the rounds is printed beside every median.  All three variants come from the same build.
Beside the times: the (row, key) pairs each variant PROCESSES, in tiles of 128 rows x 64 keys -- the gathered kernel's items walk
ceil-counted list tiles up to their last diagonal position plus their band tiles, the dense kernel the causal triangle, the
block_mask kernel two tiles per selected block -- and the time per processed tile.  The last figure of the gathered kernel against
the dense one is what gathering costs.  Reported, not asserted.
--bwd: the same for the backward (-> profiles/key_index_bwd_rates.txt): the whole gathered-key backward (band launches + dQ + dK/dV +
scatter), its halves (only="dq" / "dkdv"), the band's launches alone (the windowed causal backward), the new launches alone (the call
without a window: the listed compare e <= d_i, a little more than e < d_i - left), the dense causal backward and the block_mask
backward on the cover; every variant on the lse and delta of its own forward.  Tiles are the forward's counts: the same pairs."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seq", type=int, default=32768)
    ap.add_argument("--left", type=int, default=1023)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--bwd", action="store_true")
    a = ap.parse_args()
    from yunchang_amd import _C
    dev = torch.device("cuda:0")
    B, S, Hq, Hkv, D, left, n = 1, a.seq, 32, 4, 128, a.left, a.n
    gen = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, S, h, D, generator=gen).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv))
    lists = torch.stack([torch.randperm(S, generator=gen)[:n].sort().values for _ in range(Hq)])        # (Hq, n), host copy kept
    idx = lists.to(torch.int32).to(dev)
    # the 128-block cover of the pattern: the band's blocks, and below the diagonal every block that holds a listed key
    nb = (S + 127) // 128
    r, c = torch.arange(nb)[:, None], torch.arange(nb)[None, :]
    band = (c <= r) & (c >= (128 * r - left).clamp(min=0) // 128)
    holds = torch.zeros(Hq, nb, dtype=torch.bool)
    holds.scatter_(1, lists // 128, True)
    cover = (band[None] | (holds[:, None, :] & (c <= r)[None])).to(dev)
    out, lse = torch.empty_like(q), torch.empty(B, Hq, S, device=dev)
    scale = D ** -0.5

    # processed tiles (128 rows x 64 keys)
    nq = (S + 127) // 128
    d_hi = torch.arange(nq) * 128 + 127
    first = lists[:, ::64]                                                                  # first entry of every list tile
    n_g = (first[:, None, :] <= d_hi[None, :, None]).sum(-1)                                # (Hq, nq)
    n_b = d_hi // 64 - (d_hi - 127 - left).clamp(min=0) // 64 + 1
    tiles = {"key_index": int((n_g + n_b[None]).sum()), "dense causal": Hq * int((d_hi // 64 + 1).sum()),
             "block_mask cover": 2 * int(cover.sum())}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    variants = {
        "key_index": lambda: _C.flash_fwd(q, k, v, scale, True, lse, out=out, window=(left, 0), key_index=idx),
        "dense causal": lambda: _C.flash_fwd(q, k, v, scale, True, lse, out=out),
        "block_mask cover": lambda: _C.flash_fwd(q, k, v, scale, True, lse, out=out, bsp=cover),
    }
    if a.bwd:
        dout = torch.randn(B, S, Hq, D, generator=gen).to(torch.bfloat16).to(dev)
        g = [torch.empty_like(t) for t in (q, k, v)]

        def state(**kw):                            # the lse and delta of the variant's own forward
            lse_, out_, delta_ = torch.empty(B, Hq, S, device=dev), torch.empty_like(q), torch.empty(B, Hq, S, device=dev)
            _C.flash_fwd(q, k, v, scale, True, lse_, out=out_, **kw)
            _C.bwd_delta(dout, out_, delta_)
            return lse_, delta_

        def bwd(st, **kw):
            return lambda: _C.flash_bwd(dout, q, k, v, st[0], st[1], None, None, None, scale, True, dq16=g[0], dk16=g[1], dv16=g[2], **kw)
        sg, sn = state(window=(left, 0), key_index=idx), state(key_index=idx)
        sw, sd, sb = state(window=(left, 0)), state(), state(bsp=cover)
        variants = {"key_index": bwd(sg, window=(left, 0), key_index=idx),
                    "key_index dq": bwd(sg, window=(left, 0), key_index=idx, only="dq"),
                    "key_index dkdv": bwd(sg, window=(left, 0), key_index=idx, only="dkdv"),
                    "band dq": bwd(sw, window=(left, 0), only="dq"), "band dkdv": bwd(sw, window=(left, 0), only="dkdv"),
                    "listed dq": bwd(sn, key_index=idx, only="dq"), "listed dkdv+scatter": bwd(sn, key_index=idx, only="dkdv"),
                    "dense causal": bwd(sd), "block_mask cover": bwd(sb, bsp=cover)}
        n_band, n_list = Hq * int(n_b.sum()), int(n_g.sum())
        tiles.update({"key_index dq": tiles["key_index"], "key_index dkdv": tiles["key_index"], "band dq": n_band, "band dkdv": n_band,
                      "listed dq": n_list, "listed dkdv+scatter": n_list})
    kinds = {}
    for name, fn in variants.items():
        for _ in range(3):
            fn()
        kinds[name] = _C.last_launch_kinds()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            ms[name].append(timed(fn))
    print(f"B{B} S{S} H{Hq}/{Hkv} D{D} bf16 causal, left {left}, {n} listed keys per head (uniform); {a.rounds} rounds x {a.reps} launches, "
          f"medians [min .. max] in ms; a tile is 128 rows x 64 keys")
    med = {nm: statistics.median(t) for nm, t in ms.items()}
    for nm, t in ms.items():
        print(f"  {nm:19s} {'+'.join(kinds[nm]):32s} {med[nm]:8.3f} [{min(t):.3f} .. {max(t):.3f}] ms  {tiles[nm]:9d} tiles  "
              f"{med[nm] * 1e6 / tiles[nm]:7.2f} ns per tile")
    print(f"  key_index / dense causal: {med['key_index'] / med['dense causal']:.3f} x the time on {tiles['key_index'] / tiles['dense causal']:.3f} x "
          f"the tiles; time per tile {med['key_index'] / tiles['key_index'] / (med['dense causal'] / tiles['dense causal']):.2f} x the dense kernel's")
    print(f"  key_index / block_mask cover: {med['key_index'] / med['block_mask cover']:.3f} x the time on "
          f"{tiles['key_index'] / tiles['block_mask cover']:.3f} x the tiles (the cover also computes another function: whole blocks join the softmax)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
