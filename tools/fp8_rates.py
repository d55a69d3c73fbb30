#!/usr/bin/env python3
"""Rates of the e4m3 forward beside the 16-bit forwards of the same library, on one GPU (-> profiles/fp8_rates.txt).

    python tools/fp8_rates.py [--rounds 15] [--reps 5]

B1 S16384 H32/4 D128, causal and full.  Device events around `reps` launches, warm-up first, medians of `rounds` rounds with the
variants interleaved inside each round; the spread of the rounds is printed beside every median.  Variants: the fp8 forward
(usp_flash_fwd_fp8), the default bf16 forward (the 64-row family: the code of the parent commit, whose kernels this feature leaves
untouched) and the two-waves-per-SIMD bf16 forward (family="wave32").  Also quantize_fp8's time and bytes/s (x read twice, x8
written once), and the fp8 forward's worst error as a fraction of the bound of tests/fp8_ref.py at a size the CPU can check.
FLOPs = 4 B H S^2 D (halved under causal).  Roofs named: 2.5 PFLOP/s (bf16 MFMA), 5 PFLOP/s (fp8 MFMA), the matrix pipe in both."""
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
    a = ap.parse_args()
    from yunchang_amd import _C
    from yunchang_amd.kernels import hip_attn_forward, quantize_fp8
    import fp8_ref as R
    dev = torch.device("cuda:0")
    B, S, Hq, Hkv, D = 1, 16384, 32, 4, 128
    gen = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, S, h, D, generator=gen).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv))
    (q8, dq), (k8, dk), (v8, dv) = (quantize_fp8(x) for x in (q, k, v))
    out, lse = torch.empty_like(q), torch.empty(B, Hq, S, device=dev)
    scale = D ** -0.5

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    print(f"B{B} S{S} H{Hq}/{Hkv} D{D}, {a.rounds} rounds x {a.reps} launches, medians [min .. max] in ms")
    for causal in (True, False):
        variants = {
            "fp8": lambda: _C.flash_fwd(q8, k8, v8, scale, causal, lse, out=out, q_descale=dq, k_descale=dk, v_descale=dv),
            "bf16 default": lambda: _C.flash_fwd(q, k, v, scale, causal, lse, out=out),
            "bf16 wave32": lambda: _C.flash_fwd(q, k, v, scale, causal, lse, out=out, family="wave32"),
        }
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
        flops = 4.0 * B * Hq * S * S * D * (0.5 if causal else 1.0)
        med = {n: statistics.median(t) for n, t in ms.items()}
        for n, t in ms.items():
            roof = 5.0e15 if n == "fp8" else 2.5e15
            print(f"  {'causal' if causal else 'full  '} {n:13s} {kinds[n]!s:24s} {med[n]:8.3f} [{min(t):.3f} .. {max(t):.3f}] ms  "
                  f"{flops / med[n] * 1e-9:7.1f} TFLOP/s  {flops / med[n] / roof * 1e3:.3f} of the {roof * 1e-15:.1f} PFLOP/s MFMA roof")
        print(f"  {'causal' if causal else 'full  '} fp8 / bf16 default: {med['bf16 default'] / med['fp8']:.3f} x")
    for _ in range(3):
        quantize_fp8(q)
    tq = [timed(lambda: quantize_fp8(q)) for _ in range(a.rounds)]
    nbytes = q.numel() * (2 + 2 + 1)
    print(f"  quantize_fp8 (1, {S}, {Hq}, {D}) bf16 (two launches and three allocations): {statistics.median(tq):.3f} [{min(tq):.3f} .. {max(tq):.3f}] ms, "
          f"{nbytes / statistics.median(tq) * 1e-6:.0f} GB/s of x read twice + x8 written")
    Sc = 2048
    cq, ck, cv, cdq, cdk, cdv = q8[:, :Sc, :8], k8[:, :Sc, :1], v8[:, :Sc, :1], dq[:, :8].contiguous(), dk[:, :1].contiguous(), dv[:, :1].contiguous()
    o8, l8 = hip_attn_forward(cq, ck, cv, causal=True, q_descale=cdq, k_descale=cdk, v_descale=cdv)
    R.check(o8, l8, *R.attention(cq.cpu(), ck.cpu(), cv.cpu(), cdq.cpu(), cdk.cpu(), cdv.cpu(), scale, True),
            what=f"  fp8 forward at S{Sc} H8/1 causal (these operands)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
