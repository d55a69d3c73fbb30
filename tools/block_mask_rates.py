"""Rates of the block-sparse launches (profiles/block_mask_rates.txt): B1 S16384 H32/4 D128 bf16 causal, medians of interleaved
runs -- every round times the dense two-waves-per-SIMD launch, the all-set mask and the 1/8-density mask one after the other.

    python tools/block_mask_rates.py [rounds]

(a) all-set mask against the plain wave32 launch: the cost of the machinery; (b) a seeded random mask that keeps 1/8 of the causal
blocks, the diagonal always kept, against the same dense launch; (c) the list builder alone (usp_block_lists_build), for the forward's lists and for the backward's two families; the launch
under an all-clear mask (builder + kernels that return on empty lists) is printed beside it."""
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from yunchang_amd import _C  # noqa: E402


def main(rounds=15):
    dev = torch.device("cuda:0")
    B, S, Hq, Hkv, D = 1, 16384, 32, 4, 128
    g = torch.Generator().manual_seed(0)
    q, k, v, do = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv, Hq))
    nb = S // 128
    tril = torch.tril(torch.ones(nb, nb, dtype=torch.bool))
    sparse = ((torch.rand(B, Hq, nb, nb, generator=g) < 1 / 8) & tril) | torch.eye(nb, dtype=torch.bool)
    masks = {"dense": None, "all-set": torch.ones(nb, nb, dtype=torch.bool, device=dev), "1/8": sparse.to(dev),
             "all-clear": torch.zeros(nb, nb, dtype=torch.bool, device=dev)}
    kept = float((sparse & tril).sum()) / float(tril.sum() * B * Hq)
    scale = D ** -0.5
    out, lse = torch.empty_like(q), torch.empty((B, Hq, S), dtype=torch.float32, device=dev)
    delta = torch.empty_like(lse)
    dq, dk, dv = (torch.empty(t.shape, dtype=torch.float32, device=dev) for t in (q, k, v))

    def launch(what, m):
        kw = dict(family="wave32") if m is None else dict(bsp=m)
        if what == "fwd":
            _C.flash_fwd(q, k, v, scale, True, lse, out=out, k_splits=0, **kw)
        else:
            _C.flash_bwd(do, q, k, v, lse, delta, dq, dk, dv, scale, True, splits=(0, 0), only=what, **kw)

    times = {(w, n): [] for w in ("fwd", "dq", "dkdv") for n in masks}
    _C.flash_fwd(q, k, v, scale, True, lse, out=out, family="wave32")
    _C.bwd_delta(do, out, delta)
    for r in range(rounds + 2):
        for what in ("fwd", "dq", "dkdv"):
            for name, m in masks.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch(what, m)
                b.record()
                b.synchronize()
                if r >= 2:
                    times[what, name].append(a.elapsed_time(b))
    lists = torch.empty(_C.block_list_bytes(B, Hq, nb), dtype=torch.uint8, device=dev)
    build = {1: [], 6: []}
    for r in range(rounds + 2):
        for which in build:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _C.block_lists_build(masks["1/8"], B, Hq, S, True, lists, which)
            b.record()
            b.synchronize()
            if r >= 2:
                build[which].append(a.elapsed_time(b))
    print(f"device: {torch.cuda.get_device_name(0)}; B{B} S{S} H{Hq}/{Hkv} D{D} bf16 causal; {rounds} interleaved rounds, medians in ms")
    print(f"1/8 mask keeps {kept:.4f} of the causal blocks (diagonal included)")
    for what in ("fwd", "dq", "dkdv"):
        med = {n: statistics.median(times[what, n]) for n in masks}
        print(f"{what:5s} dense {med['dense']:.3f}  all-set {med['all-set']:.3f} ({med['all-set'] / med['dense']:.3f} x)  "
              f"1/8 {med['1/8']:.3f} ({med['1/8'] / med['dense']:.3f} x dense; {med['1/8'] / (kept * med['dense']):.2f} x the kept share)  "
              f"all-clear {med['all-clear']:.3f}  -> {'FASTER than dense' if med['1/8'] < med['dense'] else 'NOT faster than dense'}")
    print(f"builder alone (1/8 mask, (B, Hq, nb, nb) = ({B}, {Hq}, {nb}, {nb})): forward lists {statistics.median(build[1]) * 1e3:.1f} us, "
          f"dQ + dK/dV lists {statistics.median(build[6]) * 1e3:.1f} us")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 15)
