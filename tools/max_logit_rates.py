"""Rates of the max-logit launches (profiles/max_logit_rates.txt): B1 S16384 H32/4 D128 bf16 causal, medians of interleaved
rounds -- every round times the plain two-waves-per-SIMD forward, the forward with row_max, the default (64-row) forward and the
reduce one after the other.

    python tools/max_logit_rates.py [rounds] [OUT.txt]      needs an MI355X

The plain launches are this build's; tools/kernel_isa.py --every shows their kernels to be the parent commit's, instruction for
instruction, so "against the parent" is measured in one process.  With a window (128, 0) beside it: the rotated walk."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yunchang_amd import _C  # noqa: E402


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main(rounds=15, out_path=None):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    B, S, Hq, Hkv, D = 1, 16384, 32, 4, 128
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv))
    scale = D ** -0.5
    out, lse = torch.empty_like(q), torch.empty((B, Hq, S), dtype=torch.float32, device=dev)
    rm = torch.empty((B, Hq, S), dtype=torch.float32, device=dev)
    ml = torch.empty(Hq, dtype=torch.float32, device=dev)
    lines = [f"B{B} S{S} H{Hq}/{Hkv} D{D} bf16 causal, {rounds} interleaved rounds, medians (min .. max)"]
    for window, n in ((None, 10), ((128, 0), 100)):
        wl = S if window is None else window[0] + 1
        flops = 4.0 * B * Hq * sum(min(i + 1, wl) for i in range(S)) * D
        variants = {"wave32 plain": dict(family="wave32", k_splits=0), "wave32 row_max": dict(family="wave32", row_max=rm),
                    "auto row_max": dict(row_max=rm), "auto plain": dict(k_splits=0)}
        res = {}
        for name, kw in variants.items():
            run = lambda kw=kw: _C.flash_fwd(q, k, v, scale, True, lse, out=out, window=window, **kw)
            run()
            res[name] = dict(run=run, kinds=_C.last_launch_kinds(), t=[])
            for _ in range(3):
                run()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for r in res.values():
                r["t"].append(timed(r["run"], n))
        lines.append(f"window {window}")
        base, auto = statistics.median(res["wave32 plain"]["t"]), statistics.median(res["auto plain"]["t"])
        for name, r in res.items():
            t = statistics.median(r["t"])
            lines.append(f"   {name:15s} fwd {t:7.4f} ms ({min(r['t']):.4f} .. {max(r['t']):.4f}) {flops / t / 1e9:7.1f} TFLOP/s  "
                         f"{base / t:5.3f} x wave32 plain  {auto / t:5.3f} x auto plain  {r['kinds']}")
    _C.row_max_reduce(rm, out=ml)
    torch.cuda.synchronize()
    t = [timed(lambda: _C.row_max_reduce(rm, out=ml), 50) for _ in range(rounds)]
    med = statistics.median(t)
    lines.append(f"usp_row_max_reduce B{B} H{Hq} S{S}: {med * 1e3:.1f} us ({min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f}), "
                 f"{B * Hq * S * 4 / med / 1e6:.1f} GB/s of row_max")
    txt = "\n".join(lines)
    print(txt)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(txt + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 15, sys.argv[2] if len(sys.argv) > 2 else None)
