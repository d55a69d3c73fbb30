"""Rates of the document-mask kernels against the plain launch on the same family, in one process: B1 S16384 H32/Hkv4 D128 bf16
causal, the forward and the two backward launches (dK/dV and dQ) each on its own, for the plain two-waves-per-SIMD launch
(USP_FORCE_WAVE32: the yardstick), one document, eight documents of 2048 and 64 documents of random lengths.  Device events around
batches of launches, the variants alternated inside every round, medians (profiles/doc_rates.txt).

    python tools/doc_rates.py [OUT.txt]      needs an MI355X; prints one line per variant (and writes them to OUT.txt)"""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from yunchang_amd import _C
from yunchang_amd.ring import doc_blocks

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


B, S, Hq, Hkv, D = 1, 16384, 32, 4, 128
g = torch.Generator().manual_seed(0)
q, k, v, do = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv, Hq))
out = torch.empty_like(q)
lse = torch.empty(B, Hq, S, dtype=torch.float32, device=dev)
delta = torch.empty_like(lse)
dq, dk, dv = (torch.empty(t.shape, dtype=torch.float32, device=dev) for t in (q, k, v))
scale = D ** -0.5
rs = np.random.RandomState(0)
cuts = sorted(rs.choice(np.arange(1, S), size=63, replace=False).tolist())
lists = {"plain wave32": None, "1 document": [0, S], "8 x 2048": [i * 2048 for i in range(9)], "64 random": [0] + cuts + [S]}
res = {}
for name, cu in lists.items():
    doc, pairs = None, S * (S + 1) // 2
    if cu is not None:
        rl, kh = doc_blocks.block_arrays(cu, 0, S, 0, S)
        doc = (torch.from_numpy(rl).to(dev), torch.from_numpy(kh).to(dev))
        pairs = sum((e - s) * (e - s + 1) // 2 for s, e in zip(cu[:-1], cu[1:]))
    fwd = lambda doc=doc: _C.flash_fwd(q, k, v, scale, True, lse, out=out, family="wave32", k_splits=0, doc=doc)
    fwd()
    kinds = _C.last_launch_kinds()
    _C.bwd_delta(do, out, delta)
    lse_d, delta_d = lse.clone(), delta.clone()      # the rows' statistics under this mask, kept for its backward
    bwd = lambda only, doc=doc, l=lse_d, d=delta_d: _C.flash_bwd(do, q, k, v, l, d, dq, dk, dv, scale, True, family="wave32",
                                                                 splits=(0, 0), only=only, doc=doc)
    runs = {"fwd": fwd, "dkdv": lambda bwd=bwd: bwd("dkdv"), "dq": lambda bwd=bwd: bwd("dq")}
    for r in runs.values():
        for _ in range(2):
            r()
    torch.cuda.synchronize()
    res[name] = dict(runs=runs, kinds=kinds, pairs=pairs, t={w: [] for w in runs})
for rnd in range(7):                                  # alternate the variants inside every round
    for what in ("fwd", "dkdv", "dq"):
        for name, r in res.items():
            r["t"][what].append(timed(r["runs"][what], 10))
lines.append(f"B{B} S{S} H{Hq}/{Hkv} D{D} bf16 causal, family wave32, no cuts; FLOPs = B Hq D x visible (row, key) pairs x 4 (fwd) | 8 (dkdv) | 6 (dq)")
for what, mul in (("fwd", 4.0), ("dkdv", 8.0), ("dq", 6.0)):      # matrix products per visible pair: QK, PV | S, dP, dV, dK | S, dP, dQ
    base = statistics.median(res["plain wave32"]["t"][what])
    one = statistics.median(res["1 document"]["t"][what])
    for name, r in res.items():
        t = statistics.median(r["t"][what])
        lines.append(f"   {what:4s} {name:13s} {t:8.4f} ms (min {min(r['t'][what]):.4f} max {max(r['t'][what]):.4f}) "
                     f"{mul * B * Hq * D * r['pairs'] / t / 1e9:7.1f} TFLOP/s  plain / this {base / t:6.3f}  this / 1 document {t / one:6.3f}  {r['kinds'] if what == 'fwd' else ''}")
txt = "\n".join(lines)
print(txt)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write(txt + "\n")
