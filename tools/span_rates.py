"""Rates of the span kernels (usp_flash_fwd_span / usp_flash_bwd_span) against the document kernels on the same box, in one process:
B1 S16384 H32/Hkv4 D128 bf16, the forward and the two backward launches (dK/dV and dQ) each on its own, for
    doc  1 document      usp_flash_*_doc, causal, row_lo = 0: the one causal document through the document kernels
    span no span         usp_flash_*_span, the same function through the span kernels (row_lo = 0, row_hi = i + 1)
    doc  8 x 2048        eight causal documents of 2048 through the document kernels
    span 8 x 2048 bidir  eight BIDIRECTIONAL documents of 2048 (bidirectional="documents") through the span kernels
Device events around batches of launches, the variants alternated inside every round, medians; the whole measurement is made
twice ("run 1", "run 2") so that the noise is visible (profiles/span_rates.txt).

    python tools/span_rates.py [OUT.txt]      needs an MI355X; prints one line per variant and run (and writes them to OUT.txt)"""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
eight = [i * 2048 for i in range(9)]
tri = lambda n: n * (n + 1) // 2


def doc_arrays(cu):
    return dict(doc=tuple(torch.from_numpy(a).to(dev) for a in doc_blocks.block_arrays(cu, 0, S, 0, S)))


def span_arrays(cu, bidirectional):
    plan = doc_blocks.parse_plan(cu, bidirectional, 1, S)
    spans = doc_blocks.spans_of(plan)
    host = doc_blocks.span_block_arrays(plan[0] if spans else (cu or [0, S]), spans[0] if spans else (), 0, S, 0, S)
    return dict(span=tuple(torch.from_numpy(a).to(dev) for a in host))


variants = {"doc  1 document": (True, doc_arrays([0, S]), tri(S)),
            "span no span": (False, span_arrays(None, None), tri(S)),
            "doc  8 x 2048": (True, doc_arrays(eight), 8 * tri(2048)),
            "span 8 x 2048 bidir": (False, span_arrays(eight, "documents"), 8 * 2048 * 2048)}
res = {}
for name, (causal, kw, pairs) in variants.items():
    fwd = lambda causal=causal, kw=kw: _C.flash_fwd(q, k, v, scale, causal, lse, out=out, family="wave32", k_splits=0, **kw)
    fwd()
    kinds = _C.last_launch_kinds()
    _C.bwd_delta(do, out, delta)
    lse_d, delta_d = lse.clone(), delta.clone()      # the rows' statistics under this mask, kept for its backward
    bwd = lambda only, causal=causal, kw=kw, l=lse_d, d=delta_d: _C.flash_bwd(do, q, k, v, l, d, dq, dk, dv, scale, causal, family="wave32",
                                                                              splits=(0, 0), only=only, **kw)
    runs = {"fwd": fwd, "dkdv": lambda bwd=bwd: bwd("dkdv"), "dq": lambda bwd=bwd: bwd("dq")}
    for r in runs.values():
        for _ in range(2):
            r()
    torch.cuda.synchronize()
    res[name] = dict(runs=runs, kinds=kinds, pairs=pairs)
lines.append(f"B{B} S{S} H{Hq}/{Hkv} D{D} bf16, family wave32, no cuts; FLOPs = B Hq D x visible (row, key) pairs x 4 (fwd) | 8 (dkdv) | 6 (dq)")
for run in (1, 2):
    for r in res.values():
        r["t"] = {w: [] for w in r["runs"]}
    for rnd in range(7):                                  # alternate the variants inside every round
        for what in ("fwd", "dkdv", "dq"):
            for name, r in res.items():
                r["t"][what].append(timed(r["runs"][what], 10))
    for what, mul in (("fwd", 4.0), ("dkdv", 8.0), ("dq", 6.0)):
        one = statistics.median(res["doc  1 document"]["t"][what])
        for name, r in res.items():
            t = statistics.median(r["t"][what])
            lines.append(f"   run {run} {what:4s} {name:20s} {t:8.4f} ms (min {min(r['t'][what]):.4f} max {max(r['t'][what]):.4f}) "
                         f"{mul * B * Hq * D * r['pairs'] / t / 1e9:7.1f} TFLOP/s  this / doc 1 document {t / one:6.3f}  "
                         f"{r['kinds'] if what == 'fwd' else ''}")
txt = "\n".join(lines)
print(txt)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write(txt + "\n")
