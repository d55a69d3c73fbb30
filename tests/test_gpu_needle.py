"""The flash kernels on needle inputs (tests/needle_inputs.py): every key tile counted exactly once, with its own V, on the
right side of every mask edge.

On N(0,1) inputs attention is a near-uniform average: from a few thousand keys on, a lost, doubled or mispaired 64-key
tile moves no output beyond the stated tolerance (tests/test_needle_cpu.py pins that, and proves that needle inputs turn
each such defect into an error of at least 3x the bound).  Here the real kernels run on those inputs:

- the fp64 reference is tests/attn_ref_torch.py on the device; the backward follows the block contract of the other files
  (exact lse, delta from the 16-bit-rounded reference out);
- operands and NaN-prefilled outputs live in a NaN arena with guard bands (test_gpu_row64._Arena);
- the kernel kinds are asserted from `_C.last_launch_kinds()`; every launch runs twice and must be bit-identical;
- the verdict is `needle_inputs.verdicts`: golden_util's comparator with the stated tolerances (TOL, lse 2e-3 + 1e-4 |lse|,
  long_sum_atol on gradient sums of >= 1000 products) -- nothing is widened for this file.

The tables are importable without a GPU: tests/test_needle_cpu.py asserts the conditions on the inputs (needle mass, no
saturation) for every case below.  `USP_LARGE_ALL=1` adds the bench shape and fp16 variants at multi-pass depth.
The worst error / bound seen per tensor is printed by the last test of the file (`pytest -s`).
"""
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np
import pytest
import torch

import needle_inputs as NI
import shift_ref
from attn_ref_torch import ref_bwd, ref_delta, ref_fwd
from golden_util import TOL

pytestmark = pytest.mark.gpu

_ALL = os.environ.get("USP_LARGE_ALL", "0") == "1"
WORST = {}                                # tensor -> (worst err / bound, where)


class Cfg(NamedTuple):
    id: str
    B: int
    Sq: int
    Sk: int
    Hq: int
    Hkv: int
    D: int
    causal: bool
    dt: str
    family: Optional[str]                 # None: the library's own dispatch
    fwd: Optional[Tuple[str, ...]]        # kinds the forward must run (None: any one forward kind)
    bwd: Optional[Tuple[str, ...]]        # kinds the backward must run (None: one dq_ and one dkdv_ kind)
    window: Optional[Tuple[int, int]] = None
    softcap: Optional[float] = None
    q_mul: float = 1.0
    k_splits: int = 0
    splits: Tuple[int, int] = (0, 0)
    dkdv_heads: int = 0
    seed: int = 0
    shift: Optional[int] = None           # USP_ATTN_SHIFT: the diagonal of every bound at Sk - Sq + shift (None: the bit is off)
    do_mul: Optional[float] = None        # dout on ordinary rows (None: needle_inputs.do_mul_for)


_R64 = ("dkdv_row64", "dq_row64")
_W8 = ("dkdv_wave8", "dq_wave8")
_SM = "fwd_split_merge"
DENSE = [
    # ---- the three forward kinds, D in {32, 64, 128}, both 16-bit types, both families forced and the default dispatch
    Cfg("row64-causal", 1, 1024, 1024, 4, 2, 128, True, "bfloat16", "row64", ("fwd_row64",), _R64 + ("reduce_heads",)),
    Cfg("row64-fp16", 2, 512, 768, 2, 2, 128, False, "float16", "row64", ("fwd_row64",), _R64),
    Cfg("wave4-d128", 1, 1024, 1024, 4, 2, 128, True, "bfloat16", "wave32", ("fwd_wave4",), _W8 + ("reduce_heads",)),
    Cfg("wave4-d64-fp16", 1, 640, 640, 4, 4, 64, True, "float16", "wave32", ("fwd_wave4",), _W8),
    Cfg("wave4-d32", 2, 512, 512, 2, 1, 32, True, "bfloat16", "wave32", ("fwd_wave4",), _W8 + ("reduce_heads",)),
    Cfg("wave8-d128", 2, 1280, 1280, 32, 8, 128, True, "bfloat16", "wave32", ("fwd_wave8",), _W8 + ("reduce_heads",)),
    Cfg("wave8-d64", 4, 1024, 1024, 16, 4, 64, False, "bfloat16", None, ("fwd_wave8",), _W8 + ("reduce_heads",)),
    Cfg("wave8-d32-fp16", 4, 1024, 1024, 16, 16, 32, False, "float16", None, ("fwd_wave8",), _W8),
    Cfg("default-small", 1, 300, 300, 2, 2, 128, True, "bfloat16", None, ("fwd_wave4",), None),
    # ---- Sq != Sk both ways, rows without a visible key, ragged sizes
    Cfg("more-keys", 1, 384, 1000, 4, 2, 128, True, "bfloat16", "row64", ("fwd_row64",), _R64 + ("reduce_heads",)),
    Cfg("more-rows", 1, 777, 333, 2, 2, 128, True, "float16", "row64", ("fwd_row64",), _R64),
    Cfg("more-rows-w32", 1, 777, 333, 2, 1, 64, True, "bfloat16", "wave32", ("fwd_wave4",), _W8 + ("reduce_heads",)),
    Cfg("ragged", 2, 257, 255, 2, 1, 128, True, "bfloat16", "row64", ("fwd_row64",), _R64 + ("reduce_heads",)),
    Cfg("ragged-full", 1, 333, 1531, 3, 1, 128, False, "bfloat16", "wave32", ("fwd_wave4",), _W8 + ("reduce_heads",)),
    # ---- k_splits 2..8 through the binding, values that do not divide the tile count included
    Cfg("ksplit2-row64", 1, 2048, 2048, 2, 1, 128, True, "bfloat16", "row64", ("fwd_row64", _SM), _R64 + ("reduce_heads",),
        k_splits=2),
    Cfg("ksplit3-row64", 1, 1500, 1500, 2, 2, 128, True, "bfloat16", "row64", ("fwd_row64", _SM), _R64, k_splits=3),
    Cfg("ksplit5-w32", 1, 2048, 2048, 2, 2, 128, True, "float16", "wave32", None, _W8, k_splits=5),
    Cfg("ksplit7-d64", 1, 1984, 1984, 2, 1, 64, True, "bfloat16", None, None, _W8 + ("reduce_heads",), k_splits=7),
    Cfg("ksplit8-full", 1, 700, 2500, 2, 2, 128, False, "bfloat16", "row64", ("fwd_row64", _SM), _R64, k_splits=8),
    Cfg("ksplit4-window", 1, 2048, 2048, 2, 2, 128, True, "bfloat16", "wave32", None, _W8, window=(700, 0), k_splits=4),
    # ---- splits = (dq, dkdv) cuts, dkdv_heads in {1, 2, G} at G = 8
    Cfg("cuts-3-2-row64", 1, 1536, 1536, 2, 1, 128, True, "bfloat16", "row64", ("fwd_row64",),
        _R64 + ("reduce_heads", "reduce_cuts"), splits=(3, 2)),
    Cfg("cuts-5-3-w32", 1, 1400, 1900, 2, 2, 128, True, "bfloat16", "wave32", None, _W8 + ("reduce_heads", "reduce_cuts"),
        splits=(5, 3)),
    Cfg("cuts-8-4-full", 1, 1024, 2048, 2, 2, 128, False, "float16", "row64", ("fwd_row64",),
        _R64 + ("reduce_heads", "reduce_cuts"), splits=(8, 4)),
    Cfg("gqa8-heads1", 1, 1024, 1024, 8, 1, 128, True, "bfloat16", "row64", ("fwd_row64",), _R64 + ("reduce_heads",),
        dkdv_heads=1),
    Cfg("gqa8-heads2", 1, 1024, 1024, 8, 1, 128, True, "bfloat16", "wave32", ("fwd_wave4",), _W8 + ("reduce_heads",),
        dkdv_heads=2),
    Cfg("gqa8-heads8", 1, 1024, 1024, 8, 1, 128, True, "bfloat16", "row64", ("fwd_row64",), _R64, dkdv_heads=8),
    # ---- window: left only, right only, both; alone and with causal (the two-waves-per-SIMD family serves it)
    Cfg("win-left", 1, 1536, 1536, 2, 1, 128, False, "bfloat16", None, None, _W8 + ("reduce_heads",), window=(500, -1)),
    Cfg("win-right", 1, 1024, 1536, 2, 2, 128, False, "bfloat16", None, None, None, window=(-1, 300)),
    Cfg("win-both", 2, 1100, 1100, 4, 2, 64, False, "float16", None, None, _W8 + ("reduce_heads",), window=(400, 130)),
    Cfg("win-causal", 1, 2048, 2048, 2, 2, 128, True, "bfloat16", None, None, _W8, window=(777, 0)),
    # ---- softcap: q x 4 (exact), needle scores 56 nat, cap 30: the cap bites
    Cfg("softcap", 1, 1024, 1024, 4, 2, 128, True, "bfloat16", None, None, _W8 + ("reduce_heads",), softcap=30.0, q_mul=4.0),
    Cfg("softcap-d64", 1, 900, 1200, 2, 2, 64, False, "bfloat16", None, None, _W8, softcap=30.0, q_mul=4.0),
]


# ---- a shifted diagonal (USP_ATTN_SHIFT) under the causal bound and both window bounds: what one block of a windowed ring is.
# Shapes: >= 3 query tiles of 256 rows, >= 2 dK/dV blocks of 128 keys, >= 8 key tiles (2048 only where the keys are cut).
# tests/test_needle_cpu.py asserts from this table that it covers every kernel x bound x shift kind it is meant to.
def _bwd_kinds(family, G, heads=1, splits=(0, 0)):
    """dkdv_heads query heads per dK/dV item (1 where the library decides at these sizes) -> G / heads items per KV group;
    more than one slab (items x dK/dV cuts) is summed by `reduce_heads`, a cut dQ by `reduce_cuts`."""
    k = _R64 if family == "row64" else _W8
    if (G // max(1, heads)) * max(1, splits[1]) > 1:
        k += ("reduce_heads",)
    if splits[0] > 1:
        k += ("reduce_cuts",)
    return k


def _sh(id, B, Sq, Sk, Hq, Hkv, D, causal, dt, family, fwd, window, shift, **kw):
    G = Hq // Hkv
    bwd = None if family is None else _bwd_kinds(family, G, kw.get("dkdv_heads", 0) or 1, kw.get("splits", (0, 0)))
    return Cfg(id, B, Sq, Sk, Hq, Hkv, D, causal, dt, family, fwd, bwd, window=window, shift=shift, **kw)


_F64, _F4, _F8 = ("fwd_row64",), ("fwd_wave4",), ("fwd_wave8",)
SHIFTED = [
    # ---- the 64-row family: right bounds only (causal, or window_right > 0), D 128
    _sh("sh-r64-causal+70", 1, 768, 1024, 4, 2, 128, True, "bfloat16", "row64", _F64, None, 70),
    _sh("sh-r64-causal-333", 1, 1024, 768, 2, 1, 128, True, "float16", "row64", _F64, None, -333),     # rows < 589 see no key
    _sh("sh-r64-causal+128", 2, 768, 768, 2, 2, 128, True, "bfloat16", "row64", _F64, None, 128),
    _sh("sh-r64-causal-256", 1, 1024, 1280, 2, 2, 128, True, "bfloat16", "row64", _F64, None, -256),
    _sh("sh-r64-right-70", 1, 768, 900, 2, 1, 128, False, "float16", "row64", _F64, (-1, 200), -70),
    _sh("sh-r64-all-visible", 1, 640, 768, 2, 2, 128, True, "bfloat16", "row64", _F64, None, 800),     # shift >= Sk: cuts nothing
    _sh("sh-r64-ksplit3", 1, 2048, 2048, 2, 1, 128, True, "bfloat16", "row64", _F64 + (_SM,), None, 192, k_splits=3),
    _sh("sh-r64-cuts-3-2", 1, 1280, 1280, 2, 1, 128, True, "bfloat16", "row64", _F64, None, -70, splits=(3, 2)),
    _sh("sh-r64-heads1", 1, 768, 768, 4, 1, 128, True, "bfloat16", "row64", _F64, None, 64, dkdv_heads=1),
    _sh("sh-r64-heads4", 1, 768, 768, 4, 1, 128, True, "bfloat16", "row64", _F64, None, 64, dkdv_heads=4),
    # ---- the 32-row family: a left bound (the window instantiation of the forward), both bounds, causal alone; D 128, 64, 32
    _sh("sh-w4-both-100", 1, 768, 1024, 4, 2, 128, False, "bfloat16", "wave32", _F4, (200, 50), -100),
    _sh("sh-w4-left+70-d64", 1, 1024, 640, 2, 2, 64, False, "float16", "wave32", _F4, (300, -1), 70),
    _sh("sh-w4-causal-333-d32", 1, 1024, 768, 2, 1, 32, True, "bfloat16", "wave32", _F4, None, -333),
    _sh("sh-w4-narrow+37", 1, 700, 700, 2, 2, 128, True, "bfloat16", "wave32", _F4, (20, 0), 37),     # narrower than a tile
    _sh("sh-w4-all-visible-d64", 1, 640, 768, 2, 1, 64, True, "float16", "wave32", _F4, None, 768),
    _sh("sh-w4-both+256", 1, 768, 768, 2, 2, 128, True, "bfloat16", "wave32", _F4, (256, 0), 256),
    _sh("sh-w4-ksplit4-window", 1, 2048, 2048, 2, 2, 128, True, "bfloat16", "wave32", _F4 + (_SM,), (700, 0), -128, k_splits=4),
    _sh("sh-w32-cuts-5-3", 1, 1100, 1300, 2, 2, 128, True, "bfloat16", "wave32", None, None, 70, splits=(5, 3)),
    _sh("sh-w8-left-64", 2, 1024, 1024, 32, 8, 128, False, "bfloat16", "wave32", _F8, (300, -1), -64,
        do_mul=0.125),                                     # (G = 4 over 1024 rows: the rounding model's dK at 0.58 of the bound at 0.25)
    _sh("sh-w32-heads2", 1, 768, 768, 4, 1, 128, True, "bfloat16", "wave32", _F4, None, 64, dkdv_heads=2),
    # ---- the library's own dispatch
    _sh("sh-default-70", 1, 900, 900, 2, 2, 128, True, "bfloat16", None, None, None, -70, do_mul=0.125),   # (model dK 0.53 at 0.25)
]


def ring_block_cases(P=4, c=640, windows=(((639, 0), True), ((640, 0), True), ((641, 0), True), ((100, 60), False))):
    """What the basic ring really launches under a global window (ring/window_blocks.py): every distinct launch description
    (causal, window, shift) of a block that is not full, over all ranks and steps, at Sq = Sk = c -- derived from the planner,
    so a change of its decisions changes the cases."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_window_blocks", os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "long-context-attention_amd", "ring", "window_blocks.py"))
    wb = importlib.util.module_from_spec(spec)             # (by path: pure Python, importable where the package is not)
    spec.loader.exec_module(wb)
    seen = {}
    for (wl, wr), causal in windows:
        for rank in range(P):
            for step in range(P):
                blk = wb.plan_block(P, c, causal, wl, wr, rank, step)
                if blk is not None and not blk.full:
                    seen.setdefault((blk.causal, blk.window, blk.shift), None)
    out = []
    for causal, window, shift in seen:
        name = f"ring-{'causal' if causal else 'full'}-{window}-{shift}".replace(" ", "").replace("(", "").replace(")", "")
        out.append(Cfg(name, 1, c, c, 4, 2, 128, causal, "bfloat16", None, None, None, window=window, shift=shift))
    return out


RING_BLOCKS = ring_block_cases()
_CFG = {c.id: c for c in DENSE + SHIFTED + RING_BLOCKS}


def classes_for(keys_seen, D):
    """C: odd, about a quarter of the 64-key tiles a row at full depth sees (a handful of needles per row), capped by D."""
    c = max(3, min(-(-keys_seen // NI.TILE) // 4, {32: 7, 64: 15}.get(D, 61)))
    return c if c % 2 else c - 1


def _keys_seen(Sq, Sk, causal, window, shift=0):
    left, right = (-1, -1) if window is None else window
    if causal:
        right = 0
    span = (Sk if left < 0 else left) + (Sk if right < 0 else right) + 1
    seen = max(1, min(Sk, span))
    if shift and (left >= 0 or right >= 0):                # the deepest row of the shifted mask, never more than unshifted
        i = np.arange(Sq) + (Sk - Sq + int(shift))
        hi = np.minimum(Sk - 1, i + right) if right >= 0 else np.full(Sq, Sk - 1)
        lo = np.maximum(0, i - left) if left >= 0 else np.zeros(Sq, dtype=np.int64)
        seen = max(1, min(seen, int((hi - lo + 1).max())))
    return seen


def _tiles(Sq):
    return sorted({0, (Sq // 2) // 256 * 256, (Sq - 1) // 256 * 256})


def edges_for(c, k_splits=None, splits=None):
    """The edge needles of a dense case: the mask edges of sampled rows, the ends of the runs of its key and query cuts,
    the ends of 128-key dK/dV blocks."""
    rows = NI.sample_rows(c.Sq, 10, c.seed)
    sh = getattr(c, "shift", None) or 0
    e = NI.mask_edges(rows, c.Sq, c.Sk, c.causal, c.window, sh)
    ks = c.k_splits if k_splits is None else k_splits
    dqs, kvs = c.splits if splits is None else splits
    if ks > 1:
        e += NI.key_run_edges(c.Sq, c.Sk, c.causal, ks, "floor", c.window, tiles=_tiles(c.Sq), per=2, shift=sh)
    if dqs > 1:
        e += NI.key_run_edges(c.Sq, c.Sk, c.causal, dqs, "per", c.window, tiles=_tiles(c.Sq), per=2, shift=sh)
    if kvs > 1:
        e += NI.query_run_edges(c.Sq, c.Sk, c.causal, kvs, every=max(1, c.Sk // 128 // 4), per=2, shift=sh)
    e += NI.key_block_edges(c.Sq, c.Sk, c.causal, c.window, every=max(1, c.Sk // 128 // 5), per=2, shift=sh)
    return e


def make_inputs(c, k_splits=None, splits=None):
    C = classes_for(_keys_seen(c.Sq, c.Sk, c.causal, c.window, getattr(c, "shift", None) or 0), c.D)
    return NI.make(c.Sq, c.Sk, c.Hq, c.Hkv, c.D, c.dt, C, seed=c.seed, B=c.B, edges=edges_for(c, k_splits, splits),
                   q_mul=getattr(c, "q_mul", 1.0) if isinstance(c, Cfg) else 1.0, do_mul=getattr(c, "do_mul", None))


def visible_fn(c, shift=None):
    """r -> bool (Sk,): the keys row r sees.  `shift`: the case's own (None), or another one (the mutants of test_needle_cpu)."""
    left, right = (-1, -1) if c.window is None else c.window
    if c.causal:
        right = 0
    j = np.arange(c.Sk)
    sh = (getattr(c, "shift", None) or 0) if shift is None else shift
    if left < 0 and right < 0:
        sh = 0

    def vis(r):
        d = j - (r + c.Sk - c.Sq + sh)
        return (d <= right if right >= 0 else np.ones(c.Sk, bool)) & (d >= -left if left >= 0 else np.ones(c.Sk, bool))
    return vis


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from yunchang_amd import _C
    _C.load()
    return torch.device("cuda:0")


def _dev(x, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(getattr(torch, dt)).to(dev)


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def judge(what, got, want, dt, Sq, Sk, G):
    """Assert `needle_inputs.verdicts` (the suite's comparator and tolerances) and keep the worst ratio per tensor."""
    ver = NI.verdicts(got, want, dt, Sq, Sk, G)
    for n_, (ok, ratio) in ver.items():
        if ratio > WORST.get((n_, dt), (0.0, ""))[0]:
            WORST[(n_, dt)] = (ratio, what)
    print(f"[needle] {what}: " + " ".join(f"{n_}={r:.3f}" for n_, (_, r) in ver.items()))
    bad = {n_: round(r, 3) for n_, (ok, r) in ver.items() if not ok}
    assert not bad, f"{what}: out of tolerance, worst error / bound {bad}"


def _kinds_ok(kinds, want, prefixes):
    """`want` given: exactly those kinds; else exactly one kind of every prefix group (the library's own choice)."""
    if want is not None:
        return set(kinds) == set(want)
    return all(sum(k.startswith(p) for k in kinds) == 1 for p in prefixes)


def run_dense(dev, c):
    from test_gpu_row64 import _Arena
    from yunchang_amd import _C
    what = f"{c.id}: B{c.B} Sq{c.Sq} Sk{c.Sk} Hq{c.Hq} Hkv{c.Hkv} D{c.D} causal={c.causal} {c.dt} window={c.window} " \
           f"softcap={c.softcap} family={c.family} k_splits={c.k_splits} splits={c.splits} dkdv_heads={c.dkdv_heads}" \
           + ("" if c.shift is None else f" shift={c.shift}")
    nd = make_inputs(c)
    scale, G = c.D ** -0.5, c.Hq // c.Hkv
    qs, ks = (c.B, c.Sq, c.Hq, c.D), (c.B, c.Sk, c.Hkv, c.D)
    ar = _Arena(c.dt, dev, [qs, ks, ks, qs] + [qs] * 2 + [qs, ks, ks] * 2)
    tq, tk, tv, tdo = (ar.put(x) for x in (nd.q, nd.k, nd.v, nd.do))
    if c.shift is None:
        ro, rl = ref_fwd(tq, tk, tv, scale, c.causal, c.window, c.softcap)
    else:                                                  # the shifted truth (pinned to attn_ref_torch at shift 0 on the CPU)
        ro, rl = shift_ref.ref_fwd(tq, tk, tv, scale, c.causal, c.window, c.shift, c.softcap)
    if c.softcap:                                          # the cap bites: capped and uncapped exact outputs differ
        ro0, _ = ref_fwd(tq, tk, tv, scale, c.causal, c.window, None)
        diff = float((ro0 - ro).abs().max())
        assert diff > 10 * TOL[c.dt]["out"][0], f"{what}: the cap does not bite (max |capped - uncapped| = {diff:.3e})"
    kw = dict(window=c.window, softcap=c.softcap, family=c.family)
    if c.shift is not None:
        kw["shift"] = c.shift
    # ---- forward, twice ---------------------------------------------------------------------------------------------
    runs = []
    for _ in range(2):
        out = ar.out(qs)
        lse = torch.full((c.B, c.Hq, c.Sq), float("nan"), dtype=torch.float32, device=dev)
        _C.flash_fwd(tq, tk, tv, scale, c.causal, lse, out=out, k_splits=c.k_splits, **kw)
        kinds = _C.last_launch_kinds()
        assert _kinds_ok(kinds, c.fwd, (("fwd_wave", "fwd_row"),)), (what, kinds)
        assert (_SM in kinds) == (c.k_splits > 1), (what, kinds)
        runs.append((out, lse))
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]), what + ": two forward launches differ"
    out, lse = runs[0]
    fin = torch.isfinite(rl)
    assert torch.equal(torch.isfinite(lse), fin), what + ": rows without a visible key must give lse = -inf (and only they)"
    empty = (~fin).transpose(1, 2)[..., None]
    assert bool((out[empty.expand_as(out)] == 0).all()), what + ": rows without a visible key must give out = 0"
    judge(what, dict(out=out, lse=lse), dict(out=ro, lse=rl), c.dt, c.Sq, c.Sk, G)
    # ---- backward (exact lse, delta from the 16-bit-rounded reference out), twice ----------------------------------------
    o16 = ro.to(tq.dtype)
    if c.shift is None:
        rdq, rdk, rdv, delta = ref_bwd(tdo, tq, tk, tv, o16, rl, scale, c.causal, c.window, c.softcap)
    else:
        rdq, rdk, rdv = shift_ref.ref_bwd(tdo, tq, tk, tv, o16, rl, scale, c.causal, c.window, c.shift, c.softcap)
        delta = ref_delta(tdo, o16)
    lse_t, delta_t = rl.float().contiguous(), delta.float().contiguous()
    grads = []
    for _ in range(2):
        dq, dk, dv = ar.out(qs), ar.out(ks), ar.out(ks)
        _C.flash_bwd(tdo, tq, tk, tv, lse_t, delta_t, None, None, None, scale, c.causal, dq16=dq, dk16=dk, dv16=dv,
                     splits=c.splits, dkdv_heads=c.dkdv_heads, **kw)
        kinds = _C.last_launch_kinds()
        assert _kinds_ok(kinds, c.bwd, ("dq_", "dkdv_")), (what, kinds)
        grads.append((dq, dk, dv))
    assert all(_same(a, b) for a, b in zip(*grads)), what + ": two backward launches differ"
    dq, dk, dv = grads[0]
    assert bool((dq[empty.expand_as(dq)] == 0).all()), what + ": rows without a visible key must give dq = 0"
    judge(what, dict(dq=dq, dk=dk, dv=dv), dict(dq=rdq, dk=rdk, dv=rdv), c.dt, c.Sq, c.Sk, G)
    assert ar.guards_intact(), what + ": a launch wrote outside its tensors"


@pytest.mark.parametrize("c", DENSE, ids=[c.id for c in DENSE])
def test_dense_kernels_on_needle_inputs(dev, c):
    """Measured on MI355X (worst error / bound): bf16 out <= 0.27, lse <= 0.003, dq <= 0.18, dk <= 0.70, dv <= 0.62; fp16
    dq <= 0.09, dk <= 0.33, dv <= 0.14, out <= 0.30.

    FOUND WITH THIS FILE AND FIXED: `wave4-d64-fp16` (fp16, D 64, causal, the 4-wave forward) missed the fp16 `out`
    tolerance at 1.13x (the packed fp16 D 64 cases at 1.41x) on rows 64..191, lse exact to 4e-6: the pipelined loop of
    usp_flash_fwd_body.inc took the row max of the NEXT tile before that tile was masked, so a masked needle (score 20
    above the visible ones) became the reference max and every visible P went through the PV MFMA as an fp16 subnormal
    (a quantum of ~7e-4 on weights of ~1e-2).  bf16 has the range and never showed it; on N(0,1) inputs a masked score is
    never that far above the visible ones."""
    run_dense(dev, c)


@pytest.mark.parametrize("c", SHIFTED + RING_BLOCKS, ids=[c.id for c in SHIFTED + RING_BLOCKS])
def test_shifted_kernels_on_needle_inputs(dev, c):
    """The same run (kinds asserted, NaN arena, two bit-identical launches, lse = -inf / out = 0 / dq = 0 exactly on the rows
    without a visible key -- inside live launches too -- and `needle_inputs.verdicts`) with a shifted diagonal, against
    tests/shift_ref.py: an off-by-one in causal_off + shift or win_lo + shift loses or adds the private needle of a sampled
    row, a 100 % error on that row and on that key's dK / dV (tests/test_needle_cpu.py: the shift mutants).  RING_BLOCKS: the
    launches of a basic ring of 4 x 640 under the windows at which its planner's decisions flip.
    Measured on MI355X (worst error / bound; a record, not a gate -- profiles/needle_shift.txt): SHIFTED bf16 out <= 0.27,
    lse <= 0.002, dq <= 0.17, dk <= 0.48, dv <= 0.24; fp16 out <= 0.15, lse <= 0.001, dq <= 0.06, dk <= 0.21, dv <= 0.21;
    RING_BLOCKS (bf16) out <= 0.26, lse <= 0.001, dq <= 0.09, dk <= 0.25, dv <= 0.23."""
    run_dense(dev, c)


# ---------------------------------------------------------------------------------------------------------------------
# the ring-step contract: merge_in, partial final ranges, accumulating backward -- the needle mass split over two blocks
# ---------------------------------------------------------------------------------------------------------------------
RING = [
    # Sq, keys of block 1, Hq, Hkv, final_begin, final_end, dtype, family, k_splits of the second call
    (1024, 1024, 4, 2, 256, 900, "bfloat16", "row64", 0),
    (1024, 1024, 4, 2, 0, 1024, "float16", "wave32", 0),
    (768, 1536, 2, 1, 100, 513, "bfloat16", "row64", 3),
    (1280, 640, 2, 2, 0, 0, "bfloat16", None, 0),
]
RING_C = 7


def ring_inputs(Sq, Sa, Hq, Hkv, dt, seed=0):
    """q against the keys [0, Sa) (block 1, all visible) and [Sa, Sa + Sq) (block 2, causal): together causal attention
    of Sq rows over Sa + Sq keys (bottom-right), every row's needles spread over both blocks."""
    Sk = Sa + Sq
    rows = NI.sample_rows(Sq, 8, seed)
    edges = NI.mask_edges(rows, Sq, Sk, causal=True) + [(r, j) for r in rows[::3] for j in (Sa - 1, Sa)]
    return NI.make(Sq, Sk, Hq, Hkv, 128, dt, RING_C, seed=40 + seed, B=2, edges=edges)


@pytest.mark.parametrize("Sq,Sa,Hq,Hkv,fb,fe,dt,family,ks", RING)
def test_ring_step_contract_on_needle_inputs(dev, Sq, Sa, Hq, Hkv, fb, fe, dt, family, ks):
    from test_gpu_row64 import _Arena
    from yunchang_amd import _C
    B, D, Sk, G = 2, 128, Sa + Sq, Hq // Hkv
    what = f"ring step Sq{Sq} Sk{Sa}+{Sq} Hq{Hq} Hkv{Hkv} final [{fb},{fe}) {dt} family={family} k_splits={ks}"
    nd = ring_inputs(Sq, Sa, Hq, Hkv, dt)
    scale = D ** -0.5
    qs, ks_ = (B, Sq, Hq, D), (B, Sk, Hkv, D)
    ar = _Arena(dt, dev, [qs, ks_, ks_, qs, qs, qs, ks_, ks_])
    tq, tk, tv, tdo = (ar.put(x) for x in (nd.q, nd.k, nd.v, nd.do))
    ro, rl = ref_fwd(tq, tk, tv, scale, True)
    # the merge decides: neither block alone is the answer
    ro1, _ = ref_fwd(tq, tk[:, :Sa], tv[:, :Sa], scale, False)
    assert float((ro1 - ro).abs().max()) > 0.3, what + ": block 1 alone already gives the result"
    res = []
    for _ in range(2):
        out = ar.out(qs) if not res else torch.full(qs, float("nan"), dtype=tq.dtype, device=dev)
        acc = torch.full(qs, float("nan"), dtype=torch.float32, device=dev)
        lse = torch.full((B, Hq, Sq), float("nan"), dtype=torch.float32, device=dev)
        _C.flash_fwd(tq, tk[:, :Sa], tv[:, :Sa], scale, False, lse, out=None, acc=acc, final_begin=0, final_end=0,
                     family=family, k_splits=0)
        kinds1 = _C.last_launch_kinds()
        acc1 = acc.clone()
        _C.flash_fwd(tq, tk[:, Sa:], tv[:, Sa:], scale, True, lse, out=out, acc=acc, merge_in=True, final_begin=fb,
                     final_end=fe, family=family, k_splits=ks)
        kinds2 = _C.last_launch_kinds()
        res.append((out, acc, lse, acc1))
    if family == "row64":
        assert kinds1 == ("fwd_row64",) and set(kinds2) == {"fwd_row64"} | ({_SM} if ks > 1 else set()), (kinds1, kinds2)
    elif family == "wave32":
        assert kinds1[0].startswith("fwd_wave") and kinds2[0].startswith("fwd_wave"), (kinds1, kinds2)
    assert all(_same(a, b) for a, b in zip(res[0][:3], res[1][:3])), what + ": two runs differ"
    out, acc, lse, acc1 = res[0]
    fin = torch.zeros(Sq, dtype=torch.bool, device=dev)
    fin[fb:fe] = True
    judge(what + " final rows", dict(out=out[:, fin], lse=lse), dict(out=ro[:, fin], lse=rl), dt, Sq, Sk, G)
    judge(what + " running rows (fp32)", dict(out=acc[:, ~fin]), dict(out=ro[:, ~fin]), dt, Sq, Sk, G)
    assert bool(torch.isnan(out[:, ~fin]).all()), what + ": rows outside the final range must not be written to `out`"
    assert _same(acc[:, fin], acc1[:, fin]), what + ": accumulator rows of the final range must not be rewritten"
    # ---- the accumulating block backward of block 2 (global lse and delta) onto running fp32 gradients, 16-bit finals ----
    o16 = ro.to(tq.dtype)
    k2, v2 = tk[:, Sa:], tv[:, Sa:]
    rdq, rdk, rdv, delta = ref_bwd(tdo, tq, k2, v2, o16, rl, scale, True)
    # (ref_bwd's own delta is rowsum(dout * o16): the global one, as o16 is the merged out)
    lse_g, delta_g = rl.float().contiguous(), delta.float().contiguous()
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    run = [torch.randn(s, generator=gen, device=dev) for s in (qs, (B, Sq, Hkv, D), (B, Sq, Hkv, D))]
    keep = [t.clone() for t in run]
    finals = []
    for _ in range(2):
        d16 = [ar.out(s) if not finals else torch.full(s, float("nan"), dtype=tq.dtype, device=dev)
               for s in (qs, (B, Sq, Hkv, D), (B, Sq, Hkv, D))]
        _C.flash_bwd(tdo, tq, k2, v2, lse_g, delta_g, run[0], run[1], run[2], scale, True, accum_dq=True, accum_dk=True,
                     accum_dv=True, dq16=d16[0], dk16=d16[1], dv16=d16[2], family=family)
        finals.append(d16)
    assert all(_same(a, b) for a, b in zip(*finals)), what + ": two accumulating backward launches differ"
    assert all(_same(a, b) for a, b in zip(run, keep)), what + ": the running fp32 gradients must be left unchanged"
    judge(what + " accumulating backward", dict(zip(("dq", "dk", "dv"), finals[0])),
          dict(dq=keep[0].double() + rdq, dk=keep[1].double() + rdk, dv=keep[2].double() + rdv), dt, Sq, Sq, G)
    assert ar.guards_intact(), what + ": a launch wrote outside its tensors"


# ---------------------------------------------------------------------------------------------------------------------
# packed mode: unequal sequences, needles on the sequence ends and the half boundary, rows outside all sequences untouched
# ---------------------------------------------------------------------------------------------------------------------
PACKED = [
    # (first row, rows) per sequence (gaps between them belong to no sequence), Hq, Hkv, D, dtype
    (((0, 700), (700, 1348), (2100, 64), (2200, 2), (2202, 514)), 4, 2, 128, "bfloat16"),
    (((5, 130), (135, 1030), (1300, 258)), 2, 2, 64, "float16"),
]
PACKED_C = 7


def packed_inputs(seqs, Hq, Hkv, D, dt):
    T = max(s + n for s, n in seqs) + 9                    # (rows behind the last sequence too)
    edges = []
    for s0, n in seqs:
        last, half = s0 + n - 1, s0 + n // 2
        edges += [(last, last), (last, last + 1)]
        for r in sorted({half, min(last, half + 1), min(last, half + (n - n // 2) // 2), last}):
            edges += [(r, s0), (r, s0 - 1), (r, half - 1), (r, half)]
    edges = [(r, j) for r, j in edges if any(s <= r < s + n for s, n in seqs)]
    nd = NI.make(T, T, Hq, Hkv, D, dt, PACKED_C, seed=60, edges=edges, segments=list(seqs))
    return T, nd


def _packed_visible(seqs, T):
    j = np.arange(T)

    def vis(r):
        for s0, n in seqs:
            if s0 <= r < s0 + n:
                return (j >= s0) & (j <= r)
        return np.zeros(T, bool)
    return vis


@pytest.mark.parametrize("sched", [True, False], ids=["queue", "static"])
@pytest.mark.parametrize("seqs,Hq,Hkv,D,dt", PACKED, ids=["five-seqs", "three-seqs-d64-fp16"])
def test_packed_kernels_on_needle_inputs(dev, seqs, Hq, Hkv, D, dt, sched):
    from yunchang_amd import _C
    T, nd = packed_inputs(seqs, Hq, Hkv, D, dt)
    G, scale = Hq // Hkv, D ** -0.5
    what = f"packed {seqs} Hq{Hq} Hkv{Hkv} D{D} {dt} sched={sched}"
    tq, tk, tv, tdo = (_dev(x[0], dt, dev) for x in (nd.q, nd.k, nd.v, nd.do))
    tab = torch.tensor(seqs, dtype=torch.int32, device=dev)
    mx = max(n for _, n in seqs)
    inside = torch.zeros(T, dtype=torch.bool, device=dev)
    ro = torch.zeros((T, Hq, D), dtype=torch.float64, device=dev)
    rl = torch.zeros((Hq, T), dtype=torch.float64, device=dev)
    for s0, n in seqs:
        sl = slice(s0, s0 + n)
        inside[sl] = True
        o_, l_ = ref_fwd(tq[None, sl], tk[None, sl], tv[None, sl], scale, True)
        ro[sl], rl[:, sl] = o_[0], l_[0]
    o16 = ro.to(tq.dtype)
    rdq = torch.zeros_like(ro)
    rdk = torch.zeros((T, Hkv, D), dtype=torch.float64, device=dev)
    rdv = torch.zeros_like(rdk)
    for s0, n in seqs:
        sl = slice(s0, s0 + n)
        g_ = ref_bwd(tdo[None, sl], tq[None, sl], tk[None, sl], tv[None, sl], o16[None, sl], rl[None, :, sl], scale, True)
        rdq[sl], rdk[sl], rdv[sl] = g_[0][0], g_[1][0], g_[2][0]
    runs = []
    for _ in range(2):
        out = torch.full((T, Hq, D), float("nan"), dtype=tq.dtype, device=dev)
        lse = torch.full((Hq, T), float("nan"), dtype=torch.float32, device=dev)
        _C.flash_fwd_packed(tq, tk, tv, tab, tab, mx, mx, scale, True, lse, out=out, sched=sched)
        assert any(k.startswith("fwd_wave") for k in _C.last_launch_kinds()), _C.last_launch_kinds()
        runs.append((out, lse))
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]), what + ": two forward runs differ"
    out, lse = runs[0]
    assert bool(torch.isnan(out[~inside]).all()) and bool(torch.isnan(lse[:, ~inside]).all()), \
        what + ": rows outside all sequences must stay untouched"
    judge(what, dict(out=out[inside], lse=lse[:, inside]), dict(out=ro[inside], lse=rl[:, inside]), dt, mx, mx, G)
    lse_t = rl.float().contiguous()
    delta = ref_delta(tdo[None], o16[None])[0].float().contiguous()
    grads = []
    for _ in range(2):
        dq, dk, dv = (torch.full_like(t, float("nan")) for t in (tq, tk, tv))
        _C.flash_bwd_packed(tdo, tq, tk, tv, lse_t, delta, tab, tab, mx, mx, None, None, None, scale, True,
                            dq16=dq, dk16=dk, dv16=dv, sched=sched)
        grads.append((dq, dk, dv))
    assert all(_same(a, b) for a, b in zip(*grads)), what + ": two backward runs differ"
    for t in grads[0]:
        assert bool(torch.isnan(t[~inside]).all()), what + ": gradient rows outside all sequences must stay untouched"
    judge(what, {n_: t[inside] for n_, t in zip(("dq", "dk", "dv"), grads[0])},
          dict(dq=rdq[inside], dk=rdk[inside], dv=rdv[inside]), dt, mx, mx, G)
    # ---- the back halves in two steps, as a zigzag ring takes them: back rows x front keys (all visible) into fp32, then
    # back rows x back keys (causal) merged in; of the back half, its second half is final, its first half stays fp32 ----
    front = torch.tensor([(s0, n // 2) for s0, n in seqs], dtype=torch.int32, device=dev)
    back = torch.tensor([(s0 + n // 2, n - n // 2) for s0, n in seqs], dtype=torch.int32, device=dev)
    mh = (mx + 1) // 2
    out = torch.full((T, Hq, D), float("nan"), dtype=tq.dtype, device=dev)
    acc = torch.full((T, Hq, D), float("nan"), dtype=torch.float32, device=dev)
    lse = torch.full((Hq, T), float("nan"), dtype=torch.float32, device=dev)
    _C.flash_fwd_packed(tq, tk, tv, back, front, mh, mh, scale, False, lse, out=None, acc=acc, final_begin=0, final_end=0,
                        sched=sched)
    _C.flash_fwd_packed(tq, tk, tv, back, back, mh, mh, scale, True, lse, out=out, acc=acc, merge_in=True, final_begin=1,
                        final_end=2, sched=sched)
    is_final = torch.zeros(T, dtype=torch.bool, device=dev)
    is_run = torch.zeros(T, dtype=torch.bool, device=dev)
    for s0, n in seqs:
        b0, bn = s0 + n // 2, n - n // 2
        if n // 2 == 0:
            continue                                       # (a one-row sequence has no front keys: its row is not checked here)
        is_run[b0:b0 + bn // 2] = True
        is_final[b0 + bn // 2:b0 + bn] = True
    judge(what + " back halves, final rows", dict(out=out[is_final], lse=lse[:, is_final | is_run]),
          dict(out=ro[is_final], lse=rl[:, is_final | is_run]), dt, mx, mx, G)
    judge(what + " back halves, running rows (fp32)", dict(out=acc[is_run]), dict(out=ro[is_run]), dt, mx, mx, G)
    front_rows = inside.clone()
    for s0, n in seqs:
        front_rows[s0 + n // 2:s0 + n] = False
    assert bool(torch.isnan(out[~is_final]).all()), what + ": only final rows may be written to `out`"
    assert bool(torch.isnan(acc[front_rows | ~inside]).all()), what + ": rows outside the back halves must stay untouched"
    assert int(_C.sched_block(dev).abs().sum()) == 0, "the work-queue control block must be left zeroed"


# ---------------------------------------------------------------------------------------------------------------------
# multi-pass depth: the shapes of test_gpu_large_launch.CASES A, C, D, F, L -- where white noise is blind
# ---------------------------------------------------------------------------------------------------------------------
def large_needles(case):
    """The needle inputs of a case of tests/test_gpu_large_launch.py: edge needles on the mask edges and on the runs of the
    cuts the binding itself picks (`fwd_k_splits`, `bwd_splits`)."""
    from yunchang_amd import _C
    ks = _C.fwd_k_splits(case.B, case.Sq, case.Hq, case.causal) if case.k_splits is None else case.k_splits
    return make_inputs(case, k_splits=ks, splits=_C.bwd_splits(case.B, case.Sq, case.Sk, case.Hq, case.causal))


def needle_source(case, dev):
    nd = large_needles(case)
    return tuple(_dev(x, case.dt, dev) for x in (nd.q, nd.k, nd.v, nd.do))


LARGE_IDS = ("A", "C", "D", "F", "L")


@pytest.mark.parametrize("cid", LARGE_IDS)
def test_large_launch_on_needle_inputs(dev, cid):
    """`test_gpu_large_launch.run_case` itself (multi-pass asserted from the item counts, kinds, NaN arena, every element,
    twice and interleaved) with the needle inputs in place of the N(0,1) draw."""
    import test_gpu_large_launch as LL
    LL.run_case(dev, LL._BY_ID[cid], inputs=needle_source)


@pytest.mark.skipif(not _ALL, reason="USP_LARGE_ALL=1 runs the larger set")
@pytest.mark.parametrize("cid", ["bench", "A-fp16", "C-fp16", "D-fp16", "F-fp16"])
def test_large_launch_on_needle_inputs_all(dev, cid):
    import test_gpu_large_launch as LL
    LL.run_case(dev, next(c for c in LL.LARGE if c.id == cid), inputs=needle_source)


# ---------------------------------------------------------------------------------------------------------------------
# the layer: LongContextAttention's function on a virtual 2 x 4 zigzag grid, and a varlen zigzag ring
# ---------------------------------------------------------------------------------------------------------------------
GRID = dict(ud=2, rd=4, B=1, S=4096, Hq=8, Hkv=2, D=128, dt="bfloat16", C=15)


def grid_inputs():
    g = GRID
    edges = NI.mask_edges(NI.sample_rows(g["S"], 12, 5), g["S"], g["S"], causal=True)
    # the zigzag chunk boundaries (2 * rd chunks): the last key of a chunk and the first of the next
    c = g["S"] // (2 * g["rd"])
    for i in range(1, 2 * g["rd"]):
        edges += [(r, j) for r in (i * c + 17, min(g["S"] - 1, i * c + c - 1)) for j in (i * c - 1, i * c)]
    return NI.make(g["S"], g["S"], g["Hq"], g["Hkv"], g["D"], g["dt"], g["C"], seed=70, B=g["B"], edges=edges)


@pytest.fixture(scope="module")
def nccl_single():
    import torch.distributed as dist
    import yunchang_amd  # noqa: F401
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29741")
    own = not dist.is_initialized()
    if own:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    yield dist
    if own:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_layer_on_a_virtual_2x4_zigzag_grid(nccl_single, monkeypatch):
    """Every rank's output and gradients against the GLOBAL fp64 reference: with the needles of a row spread over the whole
    sequence, each rank's result depends at O(1) on every ring step and on the order of the zigzag halves."""
    from oracle import usp_oracle as O
    from virtual_grid import Ctx, VirtualGrid, patch_dist, run_grid
    g = GRID
    dev = torch.device("cuda:0")
    ud, rd, dt = g["ud"], g["rd"], g["dt"]
    ws = ud * rd
    nd = grid_inputs()
    grid = VirtualGrid(ud, rd, nccl_single)
    AL = patch_dist(monkeypatch, grid)
    monkeypatch.setattr(AL, "_FILL_ITEMS", 1)                # small tensors: let the head groups form
    import yunchang_amd.comm.relay_exchange as RX
    monkeypatch.setitem(RX._OVERRIDE, "relay", False)
    shard = lambda x, r: O.EXTRACT["zigzag"](x, r, ws, rd, ud)
    loc = [[_dev(shard(x, r), dt, dev) for x in (nd.q, nd.k, nd.v, nd.do)] for r in range(ws)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(ws)]
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        q, k, v, do = loc[r]
        upg, rpg = grid.groups_of(r)
        ctx = Ctx()
        with torch.cuda.stream(streams[r]):
            out = AL._AsyncUSPFunc.forward(ctx, q, k, v, None, True, upg, rpg, "zigzag", AL._MAX_GROUPS)
            grads = AL._AsyncUSPFunc.backward(ctx, do)[:3]
        return (out,) + tuple(grads)

    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    assert {k for k, _ in grid.calls} == {"ulysses", "ring"}
    tq, tk, tv, tdo = (_dev(x, dt, dev) for x in (nd.q, nd.k, nd.v, nd.do))
    scale = g["D"] ** -0.5
    ro, rl = ref_fwd(tq, tk, tv, scale, True)
    rdq, rdk, rdv, _ = ref_bwd(tdo, tq, tk, tv, ro.to(tq.dtype), rl, scale, True)
    want = {n_: t.cpu().numpy() for n_, t in (("out", ro), ("dq", rdq), ("dk", rdk), ("dv", rdv))}
    G = g["Hq"] // g["Hkv"]
    for r in range(ws):
        got = dict(zip(("out", "dq", "dk", "dv"), (t.float().cpu().numpy() for t in res[r])))
        judge(f"2x4 zigzag grid, rank {r}", got, {n_: shard(w, r) for n_, w in want.items()}, dt, g["S"], g["S"], G)


VARLEN = dict(P=4, lens=(768, 1280, 512), Hq=4, Hkv=2, D=128, dt="bfloat16", C=7)


def varlen_inputs():
    v = VARLEN
    cu = np.concatenate([[0], np.cumsum(v["lens"])])
    edges = []
    for s0, n in zip(cu[:-1], v["lens"]):
        c = n // (2 * v["P"])
        edges += [(s0 + n - 1, s0 + n - 1), (s0 + n - 1, s0 + n), (s0 + n // 2 + 5, s0), (s0 + n // 2 + 5, s0 - 1)]
        for i in range(1, 2 * v["P"]):                      # the zigzag chunk boundaries of every sequence
            edges += [(s0 + min(n - 1, i * c + 9), j) for j in (s0 + i * c - 1, s0 + i * c)]
    T = int(cu[-1])
    nd = NI.make(T, T, v["Hq"], v["Hkv"], v["D"], v["dt"], v["C"], seed=80, edges=[(int(r), int(j)) for r, j in edges],
                 segments=[(int(a), int(n)) for a, n in zip(cu[:-1], v["lens"])])
    return cu, nd


def test_varlen_zigzag_ring_on_needle_inputs(dev):
    """The packed ring step functions over four virtual ranks (test_gpu_parity.run_varlen_virtual_ring: the runner of the
    varlen goldens) against the global fp64 reference, lse at the block tests' tolerance."""
    from types import SimpleNamespace

    import test_gpu_parity as P
    from oracle import usp_oracle as O
    v = VARLEN
    cu, nd = varlen_inputs()
    dt, scale, ws = v["dt"], v["D"] ** -0.5, v["P"]
    tq, tk, tv, tdo = (_dev(x, dt, dev) for x in (nd.q, nd.k, nd.v, nd.do))       # (1, T, H, D)
    T = tq.shape[1]
    ro = torch.zeros((T, v["Hq"], v["D"]), dtype=torch.float64, device=dev)
    rl = torch.zeros((v["Hq"], T), dtype=torch.float64, device=dev)
    rdq, rdk, rdv = torch.zeros_like(ro), None, None
    rdk = torch.zeros((T, v["Hkv"], v["D"]), dtype=torch.float64, device=dev)
    rdv = torch.zeros_like(rdk)
    for a, b in zip(cu[:-1], cu[1:]):
        sl = slice(int(a), int(b))
        o_, l_ = ref_fwd(tq[:, sl], tk[:, sl], tv[:, sl], scale, True)
        ro[sl], rl[:, sl] = o_[0], l_[0]
        g_ = ref_bwd(tdo[:, sl], tq[:, sl], tk[:, sl], tv[:, sl], o_.to(tq.dtype), l_, scale, True)
        rdq[sl], rdk[sl], rdv[sl] = g_[0][0], g_[1][0], g_[2][0]
    shard = lambda x, r: O.zigzag_extract_local_varlen(x, cu, r, ws)
    host = lambda t: t.cpu().numpy()
    g = SimpleNamespace(name="needle varlen zigzag", ws=ws, dtype=dt, impl="zigzag", Hq=v["Hq"], Hkv=v["Hkv"], D=v["D"],
                        cu_local=cu // ws, max_local=max(v["lens"]) // ws, shard=shard,
                        q=nd.q[0], k=nd.k[0], v=nd.v[0], dout=nd.do[0],
                        out=[shard(host(ro), r) for r in range(ws)],
                        lse=[np.ascontiguousarray(shard(host(rl).T, r).T) for r in range(ws)],
                        dq=[shard(host(rdq), r) for r in range(ws)], dk=[shard(host(rdk), r) for r in range(ws)],
                        dv=[shard(host(rdv), r) for r in range(ws)])
    P.run_varlen_virtual_ring(dev, g, lse_tol=(2e-3, 1e-4))


def test_zz_worst_ratios_of_this_file():
    """Not a check of its own (`judge` asserts every ratio where it is measured): prints the worst error / bound per
    tensor and type the tests above saw."""
    for (n_, dt), (ratio, what) in sorted(WORST.items()):
        print(f"[needle-worst] {n_} {dt}: {ratio:.3f} of its bound ({what})")
