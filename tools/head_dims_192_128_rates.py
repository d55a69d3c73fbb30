"""Rates of the (192, 128) head-dim kernels (csrc/usp_flash_fwd_qk192.hip, csrc/usp_flash_bwd_qk192.hip) on one MI355X, in one
process: forward, dQ and dK/dV at B1 S16384 H16/Hkv2 bf16 causal against (a) the only way to serve the shape before them -- q, k
and v zero-padded to 256 on the D = 256 family --, (b) torch SDPA at (192, 128) where this torch build accepts it, and (c) the
library's default launches at B1 S16384 H32/Hkv4 D128, for scale.  Device events around batches of launches, the variants alternated
inside each of 15 rounds, medians; FLOPs counted at 192 + 128 dims per (row, key) (profiles/head_dims_192_128_rates.txt).

    python tools/head_dims_192_128_rates.py [OUT.txt]      needs an MI355X; prints one line per variant (and writes them to OUT.txt)"""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from yunchang_amd import _C

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
ROUNDS = 15
lines = []


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def usp_variants(tag, S, Hq, Hkv, D, Dv, pad=0):
    """fwd / dq / dkdv launches of the library at one shape (`pad`: every tensor zero-padded to that head dim, the scale kept)"""
    g = torch.Generator().manual_seed(0)
    q, k, v, do = (torch.randn(1, S, h, d, generator=g).to(torch.bfloat16).to(dev) for h, d in ((Hq, D), (Hkv, D), (Hkv, Dv), (Hq, Dv)))
    if pad:
        q, k, v, do = (torch.nn.functional.pad(t, (0, pad - t.shape[-1])) for t in (q, k, v, do))
    out, dq, dk, dv = torch.empty_like(do), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    lse = torch.empty(1, Hq, S, dtype=torch.float32, device=dev)
    delta = torch.empty_like(lse)
    scale = D ** -0.5
    fwd = lambda: _C.flash_fwd(q, k, v, scale, True, lse, out=out)
    fwd()
    kinds = {"fwd": _C.last_launch_kinds()}
    _C.bwd_delta(do, out, delta)
    runs = {"fwd": fwd}
    for name, kw in (("dq", dict(dq16=dq)), ("dkdv", dict(dk16=dk, dv16=dv))):
        runs[name] = lambda name=name, kw=kw: _C.flash_bwd(do, q, k, v, lse, delta, None, None, None, scale, True, only=name, **kw)
        runs[name]()
        kinds[name] = _C.last_launch_kinds()
    return {f"{tag} {n}": (f, kinds[n]) for n, f in runs.items()}


def sdpa_variants(S, H):
    g = torch.Generator().manual_seed(0)
    q, k, v, do = (torch.randn(1, H, S, d, generator=g).to(torch.bfloat16).to(dev) for d in (192, 192, 128, 128))
    qs, ks, vs = (t.clone().requires_grad_(True) for t in (q, k, v))
    sdpa = torch.nn.functional.scaled_dot_product_attention

    def sdpa_fwd():
        with torch.no_grad():
            sdpa(q, k, v, is_causal=True)

    def sdpa_both():
        sdpa(qs, ks, vs, is_causal=True).backward(do)
        qs.grad = ks.grad = vs.grad = None
    runs = {"torch sdpa fwd": sdpa_fwd, "torch sdpa fwd+bwd": sdpa_both}
    for f in runs.values():
        f()
    torch.cuda.synchronize()
    return {n: (f, ()) for n, f in runs.items()}


S, pairs = 16384, 16384 * 16385 // 2
# dims of matmul per (row, key): fwd S (192) + O (128); dq S + dP (128) + dQ (192); dkdv S + dP + dK (192) + dV (128)
DIMS = {"fwd": 320, "dq": 512, "dkdv": 640, "fwd+bwd": 1472}
DIMS_D128 = {"fwd": 256, "dq": 384, "dkdv": 512}    # (the D128 H32/4 lines count their own FLOPs, at 32 heads)
var = {**usp_variants("192/128 H16/2", S, 16, 2, 192, 128), **usp_variants("padded 256 H16/2", S, 16, 2, 192, 128, pad=256),
       **usp_variants("D128 H32/4", S, 32, 4, 128, 128)}
try:
    var.update(sdpa_variants(S, 16))
except Exception as e:                              # the build may refuse unequal head dims
    lines.append(f"torch sdpa at (192, 128) not timed: {repr(e)[:200]}")
times = {n: [] for n in var}
for f, _ in var.values():
    for _ in range(2):
        f()
torch.cuda.synchronize()
for rnd in range(ROUNDS):                           # alternate the variants inside every round
    for n, (f, _) in var.items():
        times[n].append(timed(f, 3))
med = {n: statistics.median(t) for n, t in times.items()}
lines.append(f"B1 S{S} bf16 causal, medians of {ROUNDS} interleaved rounds of 3 launches, device events; FLOPs at 192 + 128 dims per (row, key)")
for n, (f, kinds) in var.items():
    t = times[n]
    fl = 2.0 * pairs * (32 * DIMS_D128[n.split()[-1]] if n.startswith("D128") else 16 * DIMS[n.split()[-1]])
    lines.append(f"   {n:24s} {med[n]:8.3f} ms (min {min(t):.3f} max {max(t):.3f}) {fl / med[n] / 1e9:7.1f} TFLOP/s  {' '.join(kinds)}")
for n in ("fwd", "dq", "dkdv"):
    a, b = times["padded 256 H16/2 " + n], times["192/128 H16/2 " + n]
    lines.append(f"   192/128 {n:5s}: {statistics.median(a) / statistics.median(b):5.2f} x the padded D = 256 launch; the slowest round of the new "
                 f"kernel {max(b):.3f} ms against the fastest padded one {min(a):.3f} ms: {'faster beyond the spread' if max(b) < min(a) else 'NOT faster beyond the spread'}")
if "torch sdpa fwd" in med:
    tot = sum(med["192/128 H16/2 " + n] for n in ("fwd", "dq", "dkdv"))
    lines.append(f"   192/128 fwd {med['torch sdpa fwd'] / med['192/128 H16/2 fwd']:5.2f} x torch sdpa fwd; fwd + dq + dkdv "
                 f"{med['torch sdpa fwd+bwd'] / tot:5.2f} x torch sdpa fwd+bwd")
lines.append("multi-GPU: not measured")
txt = "\n".join(lines)
print(txt)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write(txt + "\n")
