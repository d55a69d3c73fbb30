#!/usr/bin/env python3
"""Rates and accuracy of the MXFP8 forward beside the per-head e4m3 forward and the default bf16 forward, on one GPU
(-> profiles/mxfp8_rates.txt).

    python tools/mxfp8_rates.py [--rounds 15] [--reps 5]

Timing: B1 S16384 H32/4 D128, causal and full.  Device events around `reps` launches, warm-up first, medians of `rounds` rounds with
the variants interleaved inside each round; the spread of the rounds is printed beside every median.  Variants: the MX forward
(usp_flash_fwd_mxfp8), the per-head fp8 forward (usp_flash_fwd_fp8: the parent commit's code, untouched) and the default bf16
forward.  Also quantize_fp8(mx=)'s time on both axes.  FLOPs = 4 B H S^2 D (halved under causal).
Accuracy: `out` against fp64 attention on the UNQUANTIZED bf16 inputs (S2048 H8/1, causal), for per-head fp8 and for MX, on white
noise and on an outlier input (one token in 512 and one channel in 32 multiplied by 2^6 in q, k and v): worst and RMS error over
the RMS of the reference.  Reported, not asserted."""
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
    (m_q8, m_qs), (m_k8, m_ks), (m_v8, m_vs) = (quantize_fp8(x, mx=ax) for x, ax in ((q, "d"), (k, "d"), (v, "s")))
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
            "mxfp8": lambda: _C.flash_fwd(m_q8, m_k8, m_v8, scale, causal, lse, out=out, q_descale=m_qs, k_descale=m_ks, v_descale=m_vs),
            "fp8 per head": lambda: _C.flash_fwd(q8, k8, v8, scale, causal, lse, out=out, q_descale=dq, k_descale=dk, v_descale=dv),
            "bf16 default": lambda: _C.flash_fwd(q, k, v, scale, causal, lse, out=out),
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
            print(f"  {'causal' if causal else 'full  '} {n:13s} {kinds[n]!s:16s} {med[n]:8.3f} [{min(t):.3f} .. {max(t):.3f}] ms  "
                  f"{flops / med[n] * 1e-9:7.1f} TFLOP/s")
        print(f"  {'causal' if causal else 'full  '} mxfp8 / fp8 per head: {med['mxfp8'] / med['fp8 per head']:.3f} x the time; "
              f"mxfp8 / bf16 default: {med['mxfp8'] / med['bf16 default']:.3f} x the time")
    for x, ax, name in ((q, "d", "q"), (k, "d", "k"), (v, "s", "v")):
        for _ in range(3):
            quantize_fp8(x, mx=ax)
        tq = [timed(lambda: quantize_fp8(x, mx=ax)) for _ in range(a.rounds)]
        print(f"  quantize_fp8({name} {tuple(x.shape)} bf16, mx='{ax}') (one launch, two allocations): {statistics.median(tq):.3f} "
              f"[{min(tq):.3f} .. {max(tq):.3f}] ms")

    Sc, Hc = 2048, 8
    print(f"accuracy of out against fp64 attention on the bf16 inputs, S{Sc} H{Hc}/1 causal: worst |error| and RMS error over the RMS of the reference")
    for what in ("white noise", "outliers"):
        g2 = torch.Generator().manual_seed(1)
        x = [torch.randn(1, Sc, h, D, generator=g2) for h in (Hc, 1, 1)]
        if what == "outliers":                               # one token in 512 and one channel in 32, times 2^6
            for t in x:
                t[:, 100::512] *= 64.0
                t[..., 5::32] *= 64.0
        x = [t.to(torch.bfloat16) for t in x]
        one = [torch.ones(1, t.shape[2], dtype=torch.float64) for t in x]
        ref, _, _ = R.attention(x[0].double(), x[1].double(), x[2].double(), *one, scale, True)
        xd = [t.to(dev) for t in x]
        (a8, ad), (b8, bd), (c8, cd) = (quantize_fp8(t) for t in xd)
        o_fp8, _ = hip_attn_forward(a8, b8, c8, causal=True, q_descale=ad, k_descale=bd, v_descale=cd)
        (a8, ad), (b8, bd), (c8, cd) = (quantize_fp8(t, mx=ax) for t, ax in zip(xd, "dds"))
        o_mx, _ = hip_attn_forward(a8, b8, c8, causal=True, q_descale=ad, k_descale=bd, v_descale=cd)
        o_bf, _ = hip_attn_forward(*xd, causal=True)
        rms = ref.pow(2).mean().sqrt().item()
        for name, o in (("fp8 per head", o_fp8), ("mxfp8", o_mx), ("bf16", o_bf)):
            err = o.double().cpu() - ref
            print(f"  {what:11s} {name:13s} worst {err.abs().max().item() / rms:.4f}  rms {err.pow(2).mean().sqrt().item() / rms:.5f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
