"""Rates of the softcap kernels (GPU): forward and backward of one dense causal block, timed with CUDA events.

    python tools/softcap_rates.py [--warmup 5] [--iters 20]

Shapes: B1 S16384 H32/Hkv4 bf16 causal at D = 128 and D = 64.  Each shape is timed three ways: softcap on (the
two-waves-per-SIMD softcap kernels: the 64-row family declines softcap), softcap off on the forced wave32 family (the
same family without the cap: the softcap cost itself), and softcap off unforced (what a call without softcap runs).
Prints one line per (shape, mode) with ms and TFLOP/s (causal FLOPs: fwd 2 * 2 * B * H * S^2 * D / 2, bwd 2.5 x that)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yunchang_amd import _C  # noqa: E402


def time_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S, Hq, Hkv, cap = 1, 16384, 32, 4, 30.0
    print(f"# softcap rates on {torch.cuda.get_device_name(0)}: B{B} S{S} H{Hq}/{Hkv} bf16 causal, softcap {cap}, "
          f"{args.warmup} warm-up + {args.iters} timed iterations (CUDA events)")
    for D in (128, 64):
        g = torch.Generator(device=dev).manual_seed(0)
        q = torch.randn(B, S, Hq, D, device=dev, generator=g).to(torch.bfloat16)
        k, v = (torch.randn(B, S, Hkv, D, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
        do = torch.randn_like(q)
        out = torch.empty_like(q)
        lse = torch.empty((B, Hq, S), dtype=torch.float32, device=dev)
        delta = torch.empty_like(lse)
        dq = torch.empty(q.shape, dtype=torch.float32, device=dev)
        dk16, dv16 = torch.empty_like(k), torch.empty_like(v)
        flops_f = 2 * 2 * B * Hq * S * S * D / 2
        base = {}
        for mode, family, sc in (("softcap", None, cap), ("off_wave32", "wave32", None), ("off_auto", None, None)):
            def fwd():
                _C.flash_fwd(q, k, v, D ** -0.5, True, lse, out, family=family, softcap=sc)

            def bwd():
                _C.flash_bwd(do, q, k, v, lse, delta, dq, None, None, D ** -0.5, True, dk16=dk16, dv16=dv16,
                             family=family, softcap=sc)
            fwd()
            kf = "+".join(_C.last_launch_kinds())
            _C.bwd_delta(do, out, delta)
            bwd()
            kb = "+".join(_C.last_launch_kinds())
            tf, tb = time_ms(fwd, args.warmup, args.iters), time_ms(bwd, args.warmup, args.iters)
            base[mode] = (tf, tb)
            rel = ""
            if mode != "softcap":
                rel = f"  softcap rate / this: fwd {tf / base['softcap'][0]:.2f}x  bwd {tb / base['softcap'][1]:.2f}x"
            print(f"D{D:<4d} {mode:<11s} fwd {tf:8.3f} ms {flops_f / tf / 1e9:7.1f} TFLOP/s [{kf}]   "
                  f"bwd {tb:8.3f} ms {2.5 * flops_f / tb / 1e9:7.1f} TFLOP/s [{kb}]{rel}")
        del q, k, v, do, out, dq, dk16, dv16
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
