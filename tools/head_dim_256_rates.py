"""Rates of the head-dim-256 kernels (csrc/usp_flash_fwd_d256.hip, csrc/usp_flash_bwd_d256.hip) on one MI355X, in one process:
forward, dQ and dK/dV at B1 S16384 H16/Hkv2 D256 bf16 causal against (a) the aten ops a user can run D = 256 with otherwise -- the
op behind TORCH_EFFICIENT and its backward, torch SDPA forward + backward -- and (b) the library's default launch at B1 S16384
H32/Hkv4 D128 (the 64-row family; the same FLOPs).  Then hip_attn_func forward + backward at S65536 H16/2 D256, and the worst error
of a small ragged case against the fp64 oracle as a share of the stated tolerance.  Device events around batches of launches, the
variants alternated inside each of 15 rounds, medians; FLOPs from the shapes (profiles/head_dim_256_rates.txt).

    python tools/head_dim_256_rates.py [OUT.txt]      needs an MI355X; prints one line per variant (and writes them to OUT.txt)"""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from yunchang_amd import _C
from yunchang_amd.kernels import hip_attn_func, set_head_dim_256

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


def usp_variants(tag, S, Hq, Hkv, D):
    """fwd / dq / dkdv launches of the library at one shape -> {name: (callable, kinds)}."""
    g = torch.Generator().manual_seed(0)
    q, k, v, do = (torch.randn(1, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv, Hq))
    out, dq = torch.empty_like(q), torch.empty_like(q)
    dk, dv = torch.empty_like(k), torch.empty_like(k)
    lse = torch.empty(1, Hq, S, dtype=torch.float32, device=dev)
    delta = torch.empty_like(lse)
    scale = D ** -0.5
    fwd = lambda: _C.flash_fwd(q, k, v, scale, True, lse, out=out)
    fwd()
    kinds = {"fwd": _C.last_launch_kinds()}
    _C.bwd_delta(do, out, delta)
    runs = {"fwd": fwd}
    for name, only, kw in (("dq", "dq", dict(dq16=dq)), ("dkdv", "dkdv", dict(dk16=dk, dv16=dv))):
        runs[name] = lambda only=only, kw=kw: _C.flash_bwd(do, q, k, v, lse, delta, None, None, None, scale, True, only=only, **kw)
        runs[name]()
        kinds[name] = _C.last_launch_kinds()
    return {f"{tag} {n}": (f, kinds[n]) for n, f in runs.items()}


def aten_variants(S, H, D):
    """The aten route at equal heads (K / V heads expanded, as TORCH_EFFICIENT needs them): forward and backward of both ops."""
    g = torch.Generator().manual_seed(0)
    q, k, v, do = (torch.randn(1, H, S, D, generator=g).to(torch.bfloat16).to(dev) for _ in range(4))
    eff = torch.ops.aten._scaled_dot_product_efficient_attention
    eff_bwd = torch.ops.aten._scaled_dot_product_efficient_attention_backward
    scale = D ** -0.5
    out, lse, seed, off = eff(q, k, v, None, True, 0.0, True, scale=scale)
    runs = {"aten efficient fwd": lambda: eff(q, k, v, None, True, 0.0, True, scale=scale),
            "aten efficient bwd": lambda: eff_bwd(do, q, k, v, None, out, lse, seed, off, 0.0, [True, True, True, False], True, scale=scale)}
    qs, ks, vs = (t.clone().requires_grad_(True) for t in (q, k, v))
    sdpa = torch.nn.functional.scaled_dot_product_attention

    def sdpa_fwd():
        with torch.no_grad():
            sdpa(q, k, v, is_causal=True)

    def sdpa_both():
        sdpa(qs, ks, vs, is_causal=True).backward(do)
        qs.grad = ks.grad = vs.grad = None
    runs["torch sdpa fwd"] = sdpa_fwd
    runs["torch sdpa fwd+bwd"] = sdpa_both
    for f in runs.values():
        f()
    torch.cuda.synchronize()
    return {n: (f, ()) for n, f in runs.items()}


S, pairs = 16384, 16384 * 16385 // 2
FWD = 4.0 * 16 * pairs * 256                        # = 4 * 32 * pairs * 128: both shapes
FLOPS = {"fwd": FWD, "dq": 1.5 * FWD, "dkdv": 2.0 * FWD, "bwd": 2.5 * FWD, "fwd+bwd": 3.5 * FWD}   # (dq: S, dP, dQ; dkdv: S, dP, dK, dV)
var = {**usp_variants("D256 H16/2", S, 16, 2, 256), **usp_variants("D128 H32/4", S, 32, 4, 128)}
try:
    var.update(aten_variants(S, 16, 256))
except Exception as e:                              # an op may be missing from a torch build, or refuse the head dim
    lines.append(f"aten route not timed: {repr(e)[:200]}")
times = {n: [] for n in var}
for f, _ in var.values():
    for _ in range(2):
        f()
torch.cuda.synchronize()
for rnd in range(ROUNDS):                           # alternate the variants inside every round
    for n, (f, _) in var.items():
        times[n].append(timed(f, 3))
med = {n: statistics.median(t) for n, t in times.items()}
lines.append(f"B1 S{S} bf16 causal, medians of {ROUNDS} interleaved rounds of 3 launches, device events; FLOPs from the shapes")
for n, (f, kinds) in var.items():
    t = times[n]
    fl = FLOPS[n.split()[-1]]
    lines.append(f"   {n:22s} {med[n]:8.3f} ms (min {min(t):.3f} max {max(t):.3f}) {fl / med[n] / 1e9:7.1f} TFLOP/s  {' '.join(kinds)}")
for n in ("fwd", "dq", "dkdv"):
    lines.append(f"   D256 {n:5s}: {med['D128 H32/4 ' + n] / med['D256 H16/2 ' + n]:5.3f} x the D128 rate of the same FLOPs")
if "aten efficient fwd" in med:
    bwd = med["D256 H16/2 dq"] + med["D256 H16/2 dkdv"]
    lines.append(f"   D256 fwd      : {med['aten efficient fwd'] / med['D256 H16/2 fwd']:5.2f} x aten efficient, "
                 f"{med['torch sdpa fwd'] / med['D256 H16/2 fwd']:5.2f} x torch sdpa")
    lines.append(f"   D256 dq + dkdv: {med['aten efficient bwd'] / bwd:5.2f} x aten efficient backward (one op for dq, dk and dv); "
                 f"fwd + dq + dkdv {med['torch sdpa fwd+bwd'] / (bwd + med['D256 H16/2 fwd']):5.2f} x torch sdpa fwd+bwd")
del var

# the workload-sized number: hip_attn_func forward + backward at S65536 H16/2 D256
set_head_dim_256(True)
S2 = 65536
g = torch.Generator().manual_seed(1)
q, k, v, do = (torch.randn(1, S2, h, 256, generator=g).to(torch.bfloat16).to(dev) for h in (16, 2, 2, 16))
q, k, v = (t.requires_grad_(True) for t in (q, k, v))


def step():
    hip_attn_func(q, k, v, causal=True).backward(do)
    q.grad = k.grad = v.grad = None


step()
torch.cuda.synchronize()
t = [timed(step, 1) for _ in range(5)]
fl = 3.5 * 4.0 * 16 * (S2 * (S2 + 1) // 2) * 256
lines.append(f"hip_attn_func fwd + bwd B1 S{S2} H16/2 D256 bf16 causal: {statistics.median(t):.1f} ms (min {min(t):.1f} max {max(t):.1f}), "
             f"{fl / statistics.median(t) / 1e9:.1f} TFLOP/s")
del q, k, v, do

# worst error against the fp64 oracle as a share of the stated tolerance (the ragged GQA case of tests/test_gpu_head_dim_256.py)
import needle_inputs as NI
from golden_util import round_to
from oracle import usp_oracle as O
for dt in ("bfloat16", "float16"):
    rs = np.random.RandomState(0)
    a, b_, c, d = (round_to(rs.standard_normal(s).astype(np.float32), dt) for s in [(1, 200, 3, 256), (1, 333, 1, 256), (1, 333, 1, 256), (1, 200, 3, 256)])
    tq, tk, tv, tdo = (torch.from_numpy(x).to(getattr(torch, dt)).to(dev) for x in (a, b_, c, d))
    out, lse = torch.empty_like(tq), torch.empty(1, 3, 200, dtype=torch.float32, device=dev)
    _C.flash_fwd(tq, tk, tv, 256 ** -0.5, True, lse, out=out)
    ro, rl = O.block_fwd(a, b_, c, None, True)
    o16 = round_to(ro.astype(np.float32), dt)
    delta = torch.empty_like(lse)
    _C.bwd_delta(tdo, torch.from_numpy(o16).to(getattr(torch, dt)).to(dev), delta)
    dq, dk, dv = torch.empty_like(tq), torch.empty_like(tk), torch.empty_like(tk)
    _C.flash_bwd(tdo, tq, tk, tv, torch.from_numpy(np.ascontiguousarray(rl, dtype=np.float32)).to(dev), delta, None, None, None, 256 ** -0.5, True, dq16=dq, dk16=dk, dv16=dv)
    want = dict(zip(("dq", "dk", "dv"), O.block_bwd(d, a, b_, c, o16, rl, None, True)), out=ro, lse=rl)
    got = {n: x.float().cpu().numpy() for n, x in dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv).items()}
    ver = NI.verdicts(got, want, dt, 200, 333, 3)
    lines.append(f"worst error / bound, B1 Sq200 Sk333 H3/1 D256 causal {dt}: " + " ".join(f"{n} {r:.3f}" for n, (_, r) in ver.items()))
txt = "\n".join(lines)
print(txt)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write(txt + "\n")
