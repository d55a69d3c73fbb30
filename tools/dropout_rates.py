"""Forward / backward rates of the dropout kernels (p = 0.1) against the same family without dropout (and with softcap), B1 S16384
H32/Hkv4 D128 bf16 causal: device events around batches of launches, variants alternated, repeated rounds
(profiles/dropout_rates.txt).  The backward's delta is that of the dropped `out` in every variant's own warm-up; the timed
launches do not depend on its values.

    python tools/dropout_rates.py [OUT.txt]      needs an MI355X; prints one line per variant (and writes them to OUT.txt)"""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from yunchang_amd import _C

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
B, S, Hq, Hkv, D = 1, 16384, 32, 4, 128
g = torch.Generator().manual_seed(0)
q, k, v, do = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv, Hq))
scale = D ** -0.5
out = torch.empty_like(q)
lse = torch.empty(B, Hq, S, dtype=torch.float32, device=dev)
delta = torch.empty_like(lse)
dq, dk, dv = (torch.empty(t.shape, dtype=torch.float32, device=dev) for t in (q, k, v))
fwd_flops = 4.0 * B * Hq * S * S * D / 2
bwd_flops = 2.5 * fwd_flops
variants = {"wave32 plain": dict(family="wave32"), "wave32 softcap 30": dict(family="wave32", softcap=30.0),
            "dropout 0.1": dict(dropout=(0.1, 1234, 0, 0, 0)), "auto plain (row64)": dict()}
lines = []

def fwd(kw):
    _C.flash_fwd(q, k, v, scale, True, lse, out=out, **kw)

def bwd(kw):
    _C.flash_bwd(do, q, k, v, lse, delta, dq, dk, dv, scale, True, **kw)

def timed(fn, kw, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn(kw)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n

res = {}
for name, kw in variants.items():                 # warm up every variant; note the kernels
    fwd(kw); fk = _C.last_launch_kinds()
    _C.bwd_delta(do, out, delta)
    bwd(kw); bk = _C.last_launch_kinds()
    for _ in range(3):
        fwd(kw); bwd(kw)
    torch.cuda.synchronize()
    res[name] = dict(fk=fk, bk=bk, f=[], b=[])
for rnd in range(7):                              # alternate the variants inside every round
    for name, kw in variants.items():
        res[name]["f"].append(timed(fwd, kw, 20))
        res[name]["b"].append(timed(bwd, kw, 8))
for name, r in res.items():
    f, b = statistics.median(r["f"]), statistics.median(r["b"])
    lines.append(f"{name:22s} fwd {f:7.3f} ms (min {min(r['f']):.3f} max {max(r['f']):.3f}) {fwd_flops / f / 1e9:7.1f} TFLOP/s {r['fk']}  |  "
                 f"bwd {b:7.3f} ms (min {min(r['b']):.3f} max {max(r['b']):.3f}) {bwd_flops / b / 1e9:7.1f} TFLOP/s {r['bk']}")
txt = "\n".join(lines)
print(txt)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write(txt + "\n")
