"""Forward rates of the attention-sink kernels against the same launch without sinks on the same family, in one process:
B1 S16384 H32/Hkv4 D128 causal, B1 S16384 H64/Hkv8 D64 causal with and without window (128, 0), bf16; the unforced plain rate (D128:
the 64-row family) beside them; and the time of usp_sink_bwd at B1 H32 S65536.  Device events around batches of launches, the
variants alternated inside every round, medians (profiles/sink_rates.txt).

    python tools/sink_rates.py [OUT.txt]      needs an MI355X; prints one line per variant (and writes them to OUT.txt)"""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from yunchang_amd import _C

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
lines = []


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def shape(B, S, Hq, Hkv, D, window):
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv))
    sinks = torch.linspace(-2.0, 6.0, Hq, device=dev)
    out = torch.empty_like(q)
    lse = torch.empty(B, Hq, S, dtype=torch.float32, device=dev)
    scale = D ** -0.5
    # visible (row, key) pairs: the causal triangle, or the band of window[0] + 1 keys
    wl = S if window is None else window[0] + 1
    pairs = sum(min(i + 1, wl) for i in range(S))
    flops = 4.0 * B * Hq * pairs * D
    variants = {"wave32 plain": dict(family="wave32"), "wave32 sinks": dict(family="wave32", sinks=sinks), "auto sinks": dict(sinks=sinks),
                "auto plain": dict()}
    n = 20 if window is None else 100
    res = {}
    for name, kw in variants.items():
        run = lambda kw=kw: _C.flash_fwd(q, k, v, scale, True, lse, out=out, window=window, **kw)
        run()
        kinds = _C.last_launch_kinds()
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        res[name] = dict(run=run, kinds=kinds, t=[])
    for rnd in range(7):                              # alternate the variants inside every round
        for name, r in res.items():
            r["t"].append(timed(r["run"], n))
    lines.append(f"B{B} S{S} H{Hq}/{Hkv} D{D} bf16 causal window {window}")
    base = statistics.median(res["wave32 plain"]["t"])
    for name, r in res.items():
        t = statistics.median(r["t"])
        lines.append(f"   {name:14s} fwd {t:7.4f} ms (min {min(r['t']):.4f} max {max(r['t']):.4f}) {flops / t / 1e9:7.1f} TFLOP/s "
                     f"{base / t:5.3f} x wave32 plain  {r['kinds']}")


shape(1, 16384, 32, 4, 128, None)
shape(1, 16384, 64, 8, 64, None)
shape(1, 16384, 64, 8, 64, (128, 0))

# usp_sink_bwd: B1 H32 S65536 (2 x 8 MiB read)
Bc, H, S = 1, 32, 65536
g = torch.Generator().manual_seed(1)
lse = (torch.randn(Bc, H, S, generator=g) * 2 + 8).to(dev)
delta = (torch.randn(Bc, H, S, generator=g) + 1).to(dev)
sinks = torch.linspace(-2.0, 6.0, H, device=dev)
ds = torch.empty(H, dtype=torch.float32, device=dev)
for _ in range(5):
    _C.sink_grad(sinks, lse, delta, out=ds)
torch.cuda.synchronize()
t = [timed(lambda: _C.sink_grad(sinks, lse, delta, out=ds), 50) for _ in range(7)]
med = statistics.median(t)
lines.append(f"usp_sink_bwd B{Bc} H{H} S{S}: {med * 1e3:.1f} us (min {min(t) * 1e3:.1f} max {max(t) * 1e3:.1f}), "
             f"{Bc * H * S * 8 / med / 1e6:.1f} GB/s of lse + delta")
txt = "\n".join(lines)
print(txt)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write(txt + "\n")
