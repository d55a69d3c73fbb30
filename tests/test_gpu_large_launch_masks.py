"""The document, span and sink kernels at multi-pass launch depth: every element against exact fp64 attention under the interval
mask of the GLOBAL definition (tests/interval_ref.py, on the device).

tests/test_gpu_large_launch.py holds the plain, softcap and window kernels to this; the three newest families keep the most state
per work item -- the rebased row bounds in LDS, K/V pointers, Sk and the diagonal rebased on the item's first key tile, arrays
indexed by the batch entry of a dealt item id, the sink keyed on cut 0 of a decoded item -- and their masks make whole items empty,
so one workgroup goes live -> empty -> live through the pipeline prologue.  None of that runs while a workgroup serves one item.
Every case of the table below

- declares the kernel kinds it must run (asserted from `_C.last_launch_kinds()`) and asserts from the shape, against the device's
  own CU count, that each flash launch has more items than resident workgroups (the dK/dV count from the library's workspace size);
- gives every batch entry another list (the inputs have one structure for the whole batch: an array read for the wrong entry
  changes the mask), asserts that the planner's arrays (ring/doc_blocks.py: what the kernels are handed) and the bounds of the
  definition describe one mask, and hands the arrays over as views at odd 4-byte offsets into one poisoned buffer;
- keeps operands and NaN-prefilled outputs in the guarded arena of tests/test_gpu_row64.py;
- compares every element of out / lse and -- given the exact lse and delta of the 16-bit-rounded exact out -- of dq / dk / dv through
  needle_inputs.verdicts (the project's one rule); rows that see nothing give exactly out = 0, lse = -inf (sinks: s_h), dq = 0;
- runs every launch twice and once more with `interleave=True` (one workgroup per item): bit-identical where the same kernels run,
  judged against the reference otherwise.  That comparison needs no tolerance and fails on any state carried between items.
  (Below 512 forward items of 256 rows an interleaved launch takes the 128-row shape, another kernel: DC8 and SC8 are DC and SC
  with eight entries, so that the forward of live and empty items has the bit-for-bit comparison too.)

The sink cases run the forward alone (the sinks' backward is the plain one fed another lse): unsplit, cut in two -- the sink once per
row, on cut 0 of a dealt item; the result also within tolerance of the unsplit one -- under a left window bound, on the 128-row
shape, and with Sq > Sk, where whole items see nothing and give lse = s_h.

tests/test_large_launch_masks_cpu.py shows on the CPU which item walks the table reaches, that workgroups of DC and SC serve live
items directly after empty ones and the other way round, and -- with the reference alone -- that a mask wrong by one step, read
for the wrong batch entry or stale by one tile fails these comparisons.
"""
from typing import NamedTuple, Optional, Tuple

import numpy as np
import pytest
import torch

import doc_ref
import interval_ref as IR
import needle_inputs as NI
import span_ref
import stair_inputs as SI
import test_gpu_large_launch as LL
import test_gpu_span as TS

pytestmark = pytest.mark.gpu


class MCase(NamedTuple):
    id: str
    family: str                           # "doc" | "span" | "sink"
    B: int
    Sq: int
    Sk: int
    Hq: int
    Hkv: int
    D: int
    dt: str
    causal: bool                          # the launch's causal flag (span launches: the diagonal lies in row_hi)
    fwd: Tuple[str, ...]                  # kinds the persistent forward must run
    bwd: Tuple[str, ...]                  # kinds the backward must run (sinks: forward only)
    gsub: int                             # query heads per dK/dV item (dkdv_heads = 0: what the library picks at 256 CUs)
    dkdv_heads: int = 0
    row0: int = 0                         # the launch's rows are the global positions [row0, row0 + Sq) ...
    key0: int = 0                         # ... its keys [key0, key0 + Sk) of a sequence of S_total positions
    S_total: int = 0
    window: Optional[Tuple[int, int]] = None
    k_splits: int = 0                     # (document and span launches are served uncut)
    softcap: None = None                  # (read by test_gpu_large_launch._bwd_workspace_bytes)


_W8 = ("dkdv_wave8", "dq_wave8")
_W8R = _W8 + ("reduce_heads",)
CASES = [
    MCase("DA", "doc", 5, 2048, 2048, 16, 4, 128, "bfloat16", True, ("fwd_wave8",), _W8R, 2, S_total=2048),
    MCase("DB", "doc", 7, 637, 637, 15, 15, 64, "float16", True, ("fwd_wave4",), _W8, 1, S_total=637),
    # a ring block below the diagonal: rows = global [2048, 3072), keys = [0, 2048): full, a left bound only
    MCase("DC", "doc", 5, 1024, 2048, 16, 4, 128, "bfloat16", False, ("fwd_wave8",), _W8, 4, row0=2048, key0=0, S_total=3072),
    MCase("LD", "doc", 1, 16896, 16896, 4, 1, 128, "bfloat16", True, ("fwd_wave8",), _W8R, 1, dkdv_heads=1, S_total=16896),
    MCase("SA", "span", 5, 2048, 2048, 16, 4, 128, "float16", False, ("fwd_wave8",), _W8, 4, S_total=2048),
    MCase("SB", "span", 7, 1150, 1150, 12, 6, 64, "bfloat16", False, ("fwd_wave8",), _W8, 2, S_total=1150),
    # a ring block ABOVE the diagonal: rows = global [0, 1024), keys = [1024, 3072): only a span across the boundary is seen
    MCase("SC", "span", 5, 1024, 2048, 16, 4, 128, "bfloat16", False, ("fwd_wave8",), _W8, 4, row0=0, key0=1024, S_total=3072),
    # 48 tiles a head, 288 items in runs of 36: the irregular dealing of usp_item_deal.h (it needs a tile count divisible by 8)
    MCase("LS", "span", 1, 12288, 12288, 6, 2, 128, "bfloat16", False, ("fwd_wave8",), _W8R, 1, dkdv_heads=1, S_total=12288),
    MCase("KA", "sink", 5, 2048, 2048, 16, 4, 128, "bfloat16", True, ("fwd_wave8",), (), 0, S_total=2048),
    MCase("KA2", "sink", 5, 2048, 2048, 16, 4, 128, "bfloat16", True, ("fwd_wave8", "fwd_split_merge"), (), 0, S_total=2048, k_splits=2),
    MCase("KAw", "sink", 5, 2048, 2048, 16, 4, 128, "bfloat16", True, ("fwd_wave8",), (), 0, S_total=2048, window=(300, 0)),
    MCase("KB", "sink", 7, 637, 637, 15, 15, 64, "float16", True, ("fwd_wave4",), (), 0, S_total=637),
    # Sq > Sk under causal: the first 1024 rows, four items of every head, see nothing and give lse = s_h
    MCase("KE", "sink", 5, 2048, 1024, 16, 4, 128, "bfloat16", True, ("fwd_wave8",), (), 0, S_total=2048),
    # DC and SC with eight entries: 512 forward items, from which an interleaved launch keeps the 8-wave kernel (below, it takes
    # the 128-row shape) -- the persistent forward of live and empty items is compared BIT FOR BIT with one workgroup per item
    MCase("DC8", "doc", 8, 1024, 2048, 16, 4, 128, "bfloat16", False, ("fwd_wave8",), _W8, 4, row0=2048, key0=0, S_total=3072),
    MCase("SC8", "span", 8, 1024, 2048, 16, 4, 128, "bfloat16", False, ("fwd_wave8",), _W8, 4, row0=0, key0=1024, S_total=3072),
]
BY_ID = {c.id: c for c in CASES}


# ---------------------------------------------------------------------------------------------------------------------
# the lists of every batch entry: (cu_doclens | None, spans | "documents"), in global positions
# ---------------------------------------------------------------------------------------------------------------------
def _scaled(base, S):
    """A list of tests/test_gpu_span.py for S = 1280 continued to `S`: the same offsets around further multiples of 256."""
    more = [x for m in range(1280, S, 256) for x in (m - 1, m, m + 1)]
    return sorted(set(x for x in list(base) + more if x < S))


def _span_ends(S):
    """SPANS[1280] of tests/test_gpu_span.py and, beyond, spans that end on, one before and one after multiples of 64, 128, 256."""
    out = [sp for sp in TS.SPANS[1280] if sp[1] < 1270]
    for m in range(1344, S - 70, 192):
        out += [(m - 10, m - 1), (m, m + 3)] if (m // 64) % 2 else [(m - 9, m), (m + 1, m + 63)]
    out.append((S - 10, S))
    return out


def entries(case):
    """One (cu, spans) per batch entry, every one different."""
    c, S = case, case.S_total
    if c.id in ("DC8", "SC8"):                                    # the five of DC / SC and three more
        rs = np.random.RandomState(4800)
        more = [(SI._block_list(rs, c.Sq, c.Sk, c.row0, c.key0, S, False), ()) for _ in range(3)] if c.id == "DC8" else \
               [(None, [(1000, 1030)]), ([0, 512, S], [(512, 1536)]), (None, [(255, 1025)])]
        return entries(BY_ID[c.id[:2]]) + more
    rs = np.random.RandomState(4000 + sum(map(ord, c.id)))
    if c.family == "sink":
        return [(None, ())] * c.B
    if c.id == "DA":
        return [(_scaled(TS.CU_DOCS[1280][:-1], S) + [S], ()), ([0, 200, 1700, S], ()), ([0, S], ()),
                (SI.draw_cu(rs, S, 8), ()), (SI.draw_cu(rs, S, 8), ())]
    if c.id == "DB":
        return [(TS.CU_DOCS[320][:-1] + [383, 385, 511, 512, 513, 600, S], ()), ([0, 40, 600, S], ()), ([0, S], ())] + \
               [(SI.draw_cu(rs, S, 6), ()) for _ in range(4)]
    if c.id == "DC":
        # nothing seen (a document starts with the block's first row) | only the first 300 rows see keys | every row does | drawn
        return [([0, 1000, 2048, S], ()), ([0, 700, 2348, S], ()), ([0, 129, S], ()),
                (SI._block_list(rs, c.Sq, c.Sk, c.row0, c.key0, S, False), ()),
                (SI._block_list(rs, c.Sq, c.Sk, c.row0, c.key0, S, False), ())]
    if c.id == "LD":
        return [([0, 63, 4097, 4100, 9000, 9216, 15000, S], ())]
    if c.id == "SA":
        return [(None, _span_ends(S)), (None, [(3, 5), (200, 1700), (1800, 1803)]), (None, [(5, 6), (100, 101), (2047, 2048)]),
                (_scaled(TS.CU_DOCS[1280][:-1], S) + [S], "documents"), (None, [(0, S)])]
    if c.id == "SB":
        return [(None, [sp for sp in TS.SPANS[1280] if sp[1] <= 1100] + [(1140, S)]), (TS.CU_AROUND[1280][:-2] + [S], TS.SPANS[1280][:-1]),
                (None, [(7, 8)]), (TS.CU_DOCS[1280][:-1] + [S], "documents"), (None, [(0, S)]), (None, [(100, 1000)]),
                ([0, 500, S], [(1, 499), (501, 1149)])]
    if c.id == "SC":
        # nothing seen (no span across the boundary) | only the last 300 rows see keys (above the diagonal the rows that see a key
        # are the trailing ones: those of the one span that crosses the boundary) | every row does | as ring_block_case("above")
        return [(None, [(10, 20), (900, 1024), (1024, 1100)]), (None, [(724, 1500)]), (None, [(0, 2000)]),
                (None, [(10, 20), (400, 1200), (1600, 2000)]), ([0, 300, 2500, S], [(301, 600), (800, 2400)])]
    if c.id == "LS":
        return [([0, 100, 7000, S], [(5, 6), (63, 65), (1000, 5000), (5000, 5003), (7000, 7200), (9215, 9217), (12000, S)])]
    raise KeyError(c.id)


def span_pairs(cu, spans, S):
    return list(zip(cu[:-1], cu[1:])) if isinstance(spans, str) else list(spans)


def definition_bounds(case, lists=None):
    """(row_lo, row_hi) int64 (B, Sq) from the global definition alone (tests/interval_ref.py: bounds / window_bounds)."""
    c = case
    if c.family == "sink":
        lo, hi = IR.window_bounds(c.Sq, c.Sk, c.causal, c.window)
        return np.broadcast_to(lo, (c.B, c.Sq)).copy(), np.broadcast_to(hi, (c.B, c.Sq)).copy()
    per = [IR.bounds(c.S_total, cu, span_pairs(cu or [0, c.S_total], sp, c.S_total), c.row0, c.Sq, c.key0, c.Sk)
           for cu, sp in (entries(c) if lists is None else lists)]
    return np.stack([p[0] for p in per]), np.stack([p[1] for p in per])


def planner_arrays(case):
    """What the kernels are handed (ring/doc_blocks.py), stacked over the batch: doc (row_lo, key_hi); span (row_lo, row_hi, key_lo,
    key_hi); int32 (B, n).  An entry that sees nothing is filled as the planner fills it."""
    from yunchang_amd.ring import doc_blocks
    c, per = case, []
    for cu, sp in entries(c):
        if c.family == "doc":
            a = doc_blocks.block_arrays(cu, c.row0, c.Sq, c.key0, c.Sk)
            per.append(doc_blocks.empty_arrays(c.Sq, c.Sk) if a is None else a)
        else:
            plan = doc_blocks.parse_plan(cu, sp, 1, c.S_total)
            spans = doc_blocks.spans_of(plan)
            lst, sps = (plan[0], spans[0]) if spans is not None else (tuple(cu or (0, c.S_total)), ())
            a = doc_blocks.span_block_arrays(lst, sps, c.row0, c.Sq, c.key0, c.Sk)
            per.append(doc_blocks.span_empty_arrays(c.Sq, c.Sk) if a is None else a)
    return tuple(np.stack([p[i] for p in per]) for i in range(len(per[0])))


def _canon(lo, hi):
    """Intervals with every empty one written (0, 0)."""
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    sees = lo < hi
    return np.where(sees, lo, 0), np.where(sees, hi, 0)


def assert_one_mask(case, bounds, arrays):
    """The planner's arrays and the definition's bounds describe the same mask, by rows (what the forward and the dQ launch read) and
    by keys (what the dK/dV launch reads)."""
    c = case
    off = c.Sk - c.Sq
    i, j = np.arange(c.Sq, dtype=np.int64)[None], np.arange(c.Sk, dtype=np.int64)[None]
    for a in arrays:
        assert a.dtype == np.int32 and (np.diff(a, axis=1) >= 0).all(), c.id
    if c.family == "doc":
        rl, kh = arrays
        rows = (rl, np.clip(i + 1 + off, 0, c.Sk) if c.causal else np.full_like(rl, c.Sk))
        keys = (np.clip(j - off, 0, c.Sq) if c.causal else np.zeros_like(kh), kh)
    else:
        rows, keys = (arrays[0], arrays[1]), (arrays[2], arrays[3])
    want_k = [IR.key_bounds(lo, hi, c.Sk) for lo, hi in zip(*bounds)]
    for got, want, what in ((rows, bounds, "rows"), (keys, (np.stack([w[0] for w in want_k]), np.stack([w[1] for w in want_k])), "keys")):
        g, w = _canon(*got), _canon(*want)
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), f"{c.id}: planner and definition differ by {what}"


# ---------------------------------------------------------------------------------------------------------------------
# inputs: needles on every boundary of every entry (one structure for the whole batch)
# ---------------------------------------------------------------------------------------------------------------------
def case_edges(case):
    c, out = case, set()
    if c.family == "sink":
        return NI.mask_edges(NI.sample_rows(c.Sq), c.Sq, c.Sk, c.causal, c.window)
    lo, _ = definition_bounds(c)
    for b, (cu, sp) in enumerate(entries(c)):
        glob = []
        if c.family == "doc":
            glob = doc_ref.needle_edges(cu, c.S_total)
            if c.row0 != c.key0:                                   # a block: the staircase of its own row_lo as well
                out |= set(SI.stair_edges(lo[b], c.Sq, c.Sk, c.causal))
        else:
            glob = span_ref.needle_edges(span_pairs(cu or [0, c.S_total], sp, c.S_total), c.S_total, cu)
            if cu is not None:
                glob = glob + doc_ref.needle_edges(cu, c.S_total)
        out |= {(r - c.row0, j - c.key0) for r, j in glob}
    return sorted((r, j) for r, j in out if 0 <= r < c.Sq and 0 <= j < c.Sk)


_ND = {}


def inputs(case):
    """needle_inputs.make for the case's shape (cached per process; KA, KA2 share theirs)."""
    c = case
    key = (c.family, c.B, c.Sq, c.Sk, c.Hq, c.Hkv, c.D, c.dt, c.row0, c.key0, c.window if c.family == "sink" else c.id)
    if key not in _ND:
        if len(_ND) >= 2:
            _ND.clear()
        _ND[key] = NI.make(c.Sq, c.Sk, c.Hq, c.Hkv, c.D, c.dt, C=8, seed=sum(map(ord, c.id[:2])), B=c.B, edges=case_edges(c))
    return _ND[key]


def case_sinks(case):
    return SI.draw_sinks(np.random.RandomState(77 + case.Hq), case.Hq)


# ---------------------------------------------------------------------------------------------------------------------
# the launches of a case, from its shape (usp_flash_fwd.hip launch_fwd_w, usp_flash_bwd.hip launch_dq / launch_dkdv: served uncut)
# ---------------------------------------------------------------------------------------------------------------------
def fwd_launch(case, cus=256):
    """(kind, n_items, resident slots, n_inner)."""
    kind, n, slots, n_inner, _ = LL.fwd_launch(case, cus)
    return kind, n, slots, n_inner


def dq_launch(case, cus=256):
    nblk = -(-case.Sq // 256)
    return "dq_wave8", case.B * case.Hq * nblk, cus, nblk


def dkdv_launch(case, cus=256, slabs=None):
    """`slabs`: partial slabs of the launch (G / heads per item); None: from the declared gsub."""
    G = case.Hq // case.Hkv
    slabs = G // case.gsub if slabs is None else slabs
    nblk = -(-case.Sk // 128)
    assert ("reduce_heads" in case.bwd) == (slabs > 1), case.id
    return "dkdv_wave8", case.B * case.Hkv * nblk * slabs, cus, nblk


def dkdv_slabs(case):
    """Partial slabs of the dK/dV launch, from what the library asks for (usp_flash_bwd_workspace_bytes): 1 when it asks for none."""
    ws = LL._bwd_workspace_bytes(case, case.dkdv_heads, (0, 0))
    per = 2 * case.B * case.Sk * case.Hkv * case.D * 4
    assert ws % per == 0 and ws != per, (case.id, ws)
    return max(1, ws // per)


# ---------------------------------------------------------------------------------------------------------------------
# the GPU run
# ---------------------------------------------------------------------------------------------------------------------
WORST = {}                                # case id -> {tensor: worst err / bound}
RESULTS = {}                              # case id -> what the summary line says about launches


@pytest.fixture(scope="module")
def dev():
    from yunchang_amd import _C
    _C.load()
    return torch.device("cuda:0")


def judge(case, what, got, want):
    ver = NI.verdicts(got, want, case.dt, case.Sq, case.Sk, case.Hq // case.Hkv)
    w = WORST.setdefault(case.id, {})
    for n_, (_, ratio) in ver.items():
        w[n_] = max(w.get(n_, 0.0), ratio)
    print(f"[large-masks] {what}: " + " ".join(f"{n_}={r:.3f}" for n_, (_, r) in ver.items()))
    bad = {n_: round(r, 3) for n_, (ok, r) in ver.items() if not ok}
    assert not bad, f"{what}: out of tolerance, worst error / bound {bad}"


def _poisoned_views(arrays, dev):
    """The int32 arrays as views at odd 4-byte offsets into ONE poisoned device buffer (tests/test_gpu_span.py:
    test_independent_layouts) -> (views, device buffer, host copy)."""
    poison, gap = np.int32(0x40000000), 37
    buf = np.full(sum(a.size + gap for a in arrays) + gap, poison, dtype=np.int32)
    offs, cur = [], gap
    for a in arrays:
        buf[cur:cur + a.size] = a.reshape(-1)
        offs.append(cur)
        cur += a.size + gap
    dbuf = torch.from_numpy(buf).to(dev)
    return tuple(dbuf[o:o + a.size].view(a.shape) for o, a in zip(offs, arrays)), dbuf, buf


def _empty(lo, hi, dev):
    """(B, Sq) bool on the device: rows that see nothing."""
    return torch.from_numpy(lo >= hi).to(dev)


def _check_fwd(case, what, out, lse, ref, empty, sinks):
    judge(case, what, dict(out=out, lse=lse), dict(out=ref["ro"], lse=ref["rl"]))
    e4 = empty[:, :, None, None].expand_as(out)
    assert bool((out[e4] == 0).all()), what + ": rows that see nothing must give out = 0"
    le = lse.transpose(1, 2)[empty]                                # (rows, Hq)
    if sinks is None:
        assert bool(torch.isneginf(le).all()), what + ": rows that see nothing must give lse = -inf"
        assert torch.equal(torch.isneginf(lse), empty[:, None, :].expand_as(lse)), what + ": lse = -inf on other rows"
    else:
        assert torch.equal(le, sinks[None, :].expand_as(le)), what + ": rows that see nothing must give lse = s_h"


def run_case(dev, case):
    from test_gpu_row64 import _Arena
    from yunchang_amd import _C
    c = case
    cus, G, scale = LL._cus(dev), c.Hq // c.Hkv, c.D ** -0.5
    what = f"{c.id}: {c.family} B{c.B} Sq{c.Sq} Sk{c.Sk} H{c.Hq}/{c.Hkv} D{c.D} {c.dt} causal={c.causal} window={c.window} k_splits={c.k_splits}"
    # ---- every flash launch is multi-pass ------------------------------------------------------------------------------
    fk, fn, fslots, _ = fwd_launch(c, cus)
    assert fn > fslots, (what, fk, fn, fslots)
    counts = {fk: fn}
    if c.bwd:
        _, qn, qslots, _ = dq_launch(c, cus)
        slabs = dkdv_slabs(c)
        assert slabs == (G // c.dkdv_heads if c.dkdv_heads else slabs) and G % slabs == 0, (what, slabs)
        _, kn, kslots, _ = dkdv_launch(c, cus, slabs)
        assert qn > qslots and kn > kslots, (what, qn, kn, cus)
        counts.update(dq_wave8=qn, dkdv_wave8=kn)
        if cus == 256:
            assert G // slabs == c.gsub, (what, "heads per dK/dV item", G // slabs)
    # ---- the mask: definition and planner -----------------------------------------------------------------------------
    lo, hi = definition_bounds(c)
    kw, dbuf, host = {}, None, None
    if c.family != "sink":
        arrays = planner_arrays(c)
        assert_one_mask(c, (lo, hi), arrays)
        views, dbuf, host = _poisoned_views(arrays, dev)
        kw = {c.family: views}
    sinks = torch.from_numpy(case_sinks(c)).to(dev) if c.family == "sink" else None
    if sinks is not None:
        kw = dict(sinks=sinks, window=c.window, k_splits=c.k_splits)
    nd = inputs(c)
    dt = getattr(torch, c.dt)
    q, k, v, do = (torch.from_numpy(x).to(dev).to(dt) for x in (nd.q, nd.k, nd.v, nd.do))
    ro, rl = IR.ref_fwd(q, k, v, scale, lo, hi, sinks)
    ref = dict(ro=ro, rl=rl)
    empty = _empty(lo, hi, dev)
    qs, ks = tuple(q.shape), tuple(k.shape)
    ar = _Arena(c.dt, dev, [qs, ks, ks, qs] + [qs] * 4 + ([qs, ks, ks] * 3 if c.bwd else []))
    tq, tk, tv, tdo = (ar.put(t) for t in (q, k, v, do))
    # ---- forward: twice persistent, once interleaved ------------------------------------------------------------------
    fwd = []
    for interleave in (False, False, True):
        out = ar.out(qs)
        lse = torch.full((c.B, c.Hq, c.Sq), float("nan"), dtype=torch.float32, device=dev)
        _C.flash_fwd(tq, tk, tv, scale, c.causal, lse, out=out, interleave=interleave, **kw)
        fwd.append((out, lse, _C.last_launch_kinds()))
    assert set(fwd[0][2]) == set(c.fwd), (what, fwd[0][2])
    _check_fwd(c, what + " fwd", fwd[0][0], fwd[0][1], ref, empty, sinks)
    assert fwd[1][2] == fwd[0][2] and LL._same_bits(fwd[1][0], fwd[0][0]) and LL._same_bits(fwd[1][1], fwd[0][1]), \
        what + ": two persistent forward launches differ"
    same_f = fwd[2][2] == fwd[0][2]
    if fk == "fwd_wave4" or fn >= 512:                             # (usp_flash_fwd.hip: below 512 items of 256 rows an interleaved launch takes 128)
        assert same_f, (what, fwd[2][2])
    if same_f:
        assert LL._same_bits(fwd[2][0], fwd[0][0]) and LL._same_bits(fwd[2][1], fwd[0][1]), \
            what + ": the interleaved forward launch differs from the persistent one"
    else:
        _check_fwd(c, what + f" fwd interleaved {fwd[2][2]}", fwd[2][0], fwd[2][1], ref, empty, sinks)
    res = dict(counts=counts, fwd=fwd[0][2], fwd_interleaved=fwd[2][2], fwd_bits="identical" if same_f else "other kernel: judged")
    RESULTS[c.id] = res
    if c.family == "sink" and c.k_splits > 1:
        # the K-split result against the unsplit one, at the stated tolerance: the sink is counted once, on cut 0
        o1 = ar.out(qs)
        l1 = torch.full((c.B, c.Hq, c.Sq), float("nan"), dtype=torch.float32, device=dev)
        _C.flash_fwd(tq, tk, tv, scale, c.causal, l1, out=o1, **dict(kw, k_splits=0))
        assert "fwd_split_merge" not in _C.last_launch_kinds()
        judge(c, what + " against the unsplit launch", dict(out=fwd[0][0], lse=fwd[0][1]), dict(out=o1.double(), lse=l1.double()))
    if not c.bwd:
        assert ar.guards_intact(), what + ": a launch wrote outside its tensors"
        return
    # ---- backward (exact lse, delta from the 16-bit-rounded reference out) ---------------------------------------------
    o16 = ro.to(dt)
    rdq, rdk, rdv, delta = IR.ref_bwd(do, q, k, v, o16, rl, scale, lo, hi)
    want = dict(dq=rdq, dk=rdk, dv=rdv)
    lse_t, delta_t = rl.float().contiguous(), delta.float().contiguous()
    bwd = []
    for interleave in (False, False, True):
        dq, dk, dv = ar.out(qs), ar.out(ks), ar.out(ks)
        _C.flash_bwd(tdo, tq, tk, tv, lse_t, delta_t, None, None, None, scale, c.causal, dq16=dq, dk16=dk, dv16=dv,
                     interleave=interleave, dkdv_heads=c.dkdv_heads, **kw)
        bwd.append(((dq, dk, dv), _C.last_launch_kinds()))
    assert set(bwd[0][1]) == set(c.bwd) or cus != 256, (what, bwd[0][1])
    assert {"dq_wave8", "dkdv_wave8"} <= set(bwd[0][1]) and ("reduce_heads" in bwd[0][1]) == (slabs > 1), (what, bwd[0][1])
    judge(c, what + " bwd", dict(zip(("dq", "dk", "dv"), bwd[0][0])), want)
    e4 = empty[:, :, None, None].expand_as(bwd[0][0][0])
    assert bool((bwd[0][0][0][e4] == 0).all()), what + ": rows that see nothing must give dq = 0"
    assert bwd[1][1] == bwd[0][1] and all(LL._same_bits(a, b) for a, b in zip(bwd[1][0], bwd[0][0])), \
        what + ": two persistent backward launches differ"
    same_b = bwd[2][1] == bwd[0][1]
    if same_b:
        assert all(LL._same_bits(a, b) for a, b in zip(bwd[2][0], bwd[0][0])), \
            what + ": the interleaved backward launches differ from the persistent ones"
    else:
        judge(c, what + f" bwd interleaved {bwd[2][1]}", dict(zip(("dq", "dk", "dv"), bwd[2][0])), want)
    res.update(bwd=bwd[0][1], bwd_bits="identical" if same_b else "other kernel: judged")
    torch.cuda.synchronize()
    assert ar.guards_intact(), what + ": a launch wrote outside its tensors"
    assert torch.equal(dbuf.cpu(), torch.from_numpy(host)), what + ": the arrays' buffer was written"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_large_launch_masks(dev, case):
    run_case(dev, case)


def test_zz_report():
    """Not a check of its own: one line per case with the launches seen and the worst error / bound per tensor."""
    for cid, w in WORST.items():
        r = RESULTS.get(cid, {})
        print(f"[large-masks-worst] {cid}: " + " ".join(f"{n_}={x:.3f}" for n_, x in w.items()) +
              f" | items {r.get('counts')} | fwd {r.get('fwd')} interleaved {r.get('fwd_interleaved')} ({r.get('fwd_bits')})"
              f" | bwd {r.get('bwd')} ({r.get('bwd_bits')})")
