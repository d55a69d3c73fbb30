"""CPU checks of what tests/test_gpu_large_launch_masks.py stands on:

1. the chunked fp64 reference for interval masks (tests/interval_ref.py) against the dense ones (tests/span_ref.py, tests/doc_ref.py,
   tests/sink_ref.py) to 1e-10, in one chunk and in chunks of a few rows;
2. the table: the planner's arrays and the definition's bounds describe one mask (for the shapes that fit, pair by pair against
   span_ref.global_mask); which item walks (the compiled usp_item_deal.h) its launches take at 256 CUs; in DC and SC workgroups
   serve a live item directly after an empty one and an empty one directly after a live one, in all three launches;
3. the comparisons of the GPU file can fail, shown with the reference alone: a list wrong by one position, the arrays of two batch
   entries exchanged, the bounds of one 256-row query tile or one 128-key block stale by one tile -- every such change that changes
   the mask fails needle_inputs.verdicts on at least one tensor."""
import numpy as np
import pytest
import torch

import doc_ref
import interval_ref as IR
import needle_inputs as NI
import sink_ref
import span_ref
import test_gpu_large_launch_masks as M
from golden_util import assert_close
from test_large_launch_cpu import _walk, walk_lib  # noqa: F401  (walk_lib: the fixture that compiles usp_item_deal.h)


def _draw(B, Sq, Sk, Hq, Hkv, D, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(torch.bfloat16) for s in [(B, Sq, Hq, D), (B, Sk, Hkv, D), (B, Sk, Hkv, D), (B, Sq, Hq, D)]]


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------
# (id, S_total, row0, Sq, key0, Sk, Hq, Hkv, D, [(cu, spans) per batch entry]): GQA, Sq != Sk, rows and whole entries that see nothing
REF_CASES = [
    ("span-whole", 40, 0, 40, 0, 40, 4, 2, 16, [(None, [(3, 9), (9, 11), (30, 40)]), ([0, 7, 25, 40], [(1, 6), (8, 20)])]),
    ("span-documents", 37, 0, 37, 0, 37, 6, 2, 16, [([0, 5, 6, 30, 37], "documents")]),
    ("span-above", 96, 0, 32, 32, 64, 4, 1, 16, [(None, [(2, 5), (20, 50)]), (None, [(1, 30), (40, 60)]), ([0, 10, 96], [(12, 90)])]),
    ("span-below", 96, 64, 32, 0, 64, 4, 2, 32, [([0, 30, 70, 96], [(31, 40), (72, 80)]), (None, [(60, 90)]), ([0, 64, 96], [])]),
    ("doc-whole", 45, 0, 45, 0, 45, 8, 2, 16, [([0, 1, 2, 17, 45], []), ([0, 45], []), ([0, 31, 32, 45], [])]),
    ("doc-below", 90, 50, 40, 3, 30, 4, 4, 16, [([0, 10, 60, 90], []), ([0, 40, 90], []), ([0, 90], [])]),
]


@pytest.mark.parametrize("chunk", [IR.CHUNK_BYTES, 3000])
@pytest.mark.parametrize("case", REF_CASES, ids=[c[0] for c in REF_CASES])
def test_interval_reference_matches_span_and_doc_ref(case, chunk):
    name, S, row0, Sq, key0, Sk, Hq, Hkv, D, lists = case
    B = len(lists)
    q, k, v, do = _draw(B, Sq, Sk, Hq, Hkv, D, seed=S + Sq)
    scale = D ** -0.5
    per = [IR.bounds(S, cu, M.span_pairs(cu or [0, S], sp, S), row0, Sq, key0, Sk) for cu, sp in lists]
    lo, hi = np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
    if name.startswith("span"):
        mask = torch.cat([span_ref.global_mask(S, cu, M.span_pairs(cu or [0, S], sp, S)) for cu, sp in lists])
        want = span_ref.ref_bwd(do, q, k, v, scale, mask[:, row0:row0 + Sq, key0:key0 + Sk], out_dtype=q.dtype)
    else:
        mask = torch.cat([doc_ref.global_mask(cu, S) for cu, _ in lists])
        want = doc_ref.ref_bwd(do, q, k, v, scale, mask[:, row0:row0 + Sq, key0:key0 + Sk], out_dtype=q.dtype)
    empty = ~torch.isfinite(want[1])                                   # (B, Hq, Sq)
    if name in ("span-above", "span-below", "doc-below"):
        assert bool(empty.any()) and bool(empty.all(-1).all(-1).any()) and not bool(empty.all())   # rows and a whole entry see nothing
    ro, rl = IR.ref_fwd(q, k, v, scale, lo, hi, chunk_bytes=chunk)
    assert ro.dtype == torch.float64 and rl.dtype == torch.float64
    assert_close(rl, want[1], 1e-10, 1e-10, "lse")                     # (-inf == -inf passes; anything else at -inf fails)
    assert_close(ro, want[0], 1e-10, 1e-10, "out")
    assert bool((ro.permute(0, 2, 1, 3)[empty] == 0).all())
    dq, dk, dv, _ = IR.ref_bwd(do, q, k, v, ro.to(q.dtype), rl, scale, lo, hi, chunk_bytes=chunk)
    for g_, w_, n_ in zip((dq, dk, dv), want[2:], ("dq", "dk", "dv")):
        assert_close(g_, w_, 1e-10, 1e-10, n_)
    assert bool((dq.permute(0, 2, 1, 3)[empty] == 0).all())


@pytest.mark.parametrize("chunk", [IR.CHUNK_BYTES, 3000])
@pytest.mark.parametrize("Sq,Sk,Hq,Hkv,causal,window", [(40, 40, 4, 2, True, None), (50, 30, 6, 2, True, None), (33, 47, 4, 4, True, (7, 0)),
                                                       (45, 45, 4, 1, False, (6, 3)), (60, 30, 2, 1, True, (9, 0))])
def test_interval_reference_matches_sink_ref(Sq, Sk, Hq, Hkv, causal, window, chunk):
    """With a sink per head; Sq > Sk under causal: rows that see nothing give lse = s_h and out = 0."""
    D, B = 16, 2
    q, k, v, do = _draw(B, Sq, Sk, Hq, Hkv, D, seed=Sq * 3 + Sk)
    sinks = torch.tensor([12.0, -30.0, 0.0, 3.0, 1.5, -2.0][:Hq])
    scale = D ** -0.5
    lo, hi = IR.window_bounds(Sq, Sk, causal, window)
    for s in (sinks, None):
        want = sink_ref.ref_bwd(do, q, k, v, scale, s, causal, window, out_dtype=q.dtype)
        ro, rl = IR.ref_fwd(q, k, v, scale, lo, hi, s, chunk_bytes=chunk)
        assert_close(rl, want[1], 1e-10, 1e-10, "lse")
        assert_close(ro, want[0], 1e-10, 1e-10, "out")
        rows = torch.from_numpy(lo >= hi)
        if Sq > Sk and causal:
            assert bool(rows.any())
            if s is not None:
                assert torch.equal(rl[:, :, rows], s.double()[None, :, None].expand(B, Hq, int(rows.sum())))
            assert bool((ro[:, rows] == 0).all())
        dq, dk, dv, _ = IR.ref_bwd(do, q, k, v, ro.to(q.dtype), rl, scale, lo, hi, chunk_bytes=chunk)
        for g_, w_, n_ in zip((dq, dk, dv), want[2:5], ("dq", "dk", "dv")):
            assert_close(g_, w_, 1e-10, 1e-10, n_)


def test_interval_chunks_cover_every_row_once_and_every_visible_key():
    rs = np.random.RandomState(3)
    for Sq, Sk, Hq in [(1000, 1000, 4), (700, 300, 2), (64, 64, 1), (513, 900, 3)]:
        for monotone in (True, False):
            lo = rs.randint(0, Sk + 1, size=Sq)
            hi = np.minimum(Sk, lo + rs.randint(0, 200, size=Sq) * (rs.rand(Sq) < 0.8))
            if monotone:
                lo, hi = np.sort(lo), np.sort(hi)
            for budget in (8 * Hq * 100, 8 * Hq * 5000, IR.CHUNK_BYTES):
                rows = []
                for r0, r1, k0, k1 in IR._chunks(lo, hi, Hq, budget):
                    rows.extend(range(r0, r1))
                    assert (r1 - r0) == 1 or 8 * Hq * (r1 - r0) * (k1 - k0) <= budget
                    a, b = lo[r0:r1], hi[r0:r1]
                    sees = a < b
                    assert not sees.any() or (a[sees].min() >= k0 and b[sees].max() <= k1)   # nothing visible outside the key range
                assert rows == list(range(Sq))


# ---- 2. the table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in M.CASES if c.family != "sink"], ids=lambda c: c.id)
def test_planner_and_definition_describe_one_mask(case):
    c = case
    lo, hi = M.definition_bounds(c)
    arrays = M.planner_arrays(c)
    M.assert_one_mask(c, (lo, hi), arrays)
    lists = M.entries(c)
    assert len(lists) == c.B and len({repr(x) for x in lists}) == c.B, "every batch entry has another list"
    assert len({(tuple(a), tuple(b)) for a, b in zip(lo, hi)}) == c.B, "every batch entry has another mask"
    if c.S_total > 3072:
        return
    for b, (cu, sp) in enumerate(lists):                               # pair by pair, from span_ref.global_mask
        full = span_ref.global_mask(c.S_total, cu, M.span_pairs(cu or [0, c.S_total], sp, c.S_total))
        want = full[:, c.row0:c.row0 + c.Sq, c.key0:c.key0 + c.Sk]
        assert torch.equal(span_ref.block_mask(lo[b], hi[b], c.Sq, c.Sk), want), (c.id, b)
        if c.family == "doc":
            assert torch.equal(doc_ref.block_mask(arrays[0][b], c.Sq, c.Sk, c.causal), want), (c.id, b)
            assert torch.equal(doc_ref.mask_of_key_hi(arrays[1][b], c.Sq, c.Sk, c.causal), want), (c.id, b)
        else:
            assert torch.equal(span_ref.block_mask(arrays[0][b], arrays[1][b], c.Sq, c.Sk), want), (c.id, b)
            assert torch.equal(span_ref.mask_of_keys(arrays[2][b], arrays[3][b], c.Sq, c.Sk), want), (c.id, b)


def test_lists_hold_what_the_cases_are_for():
    """DA / SA: an interior of about 1500 positions (the pipelined loop), an entry that is plain causal through the arrays, for SA
    one span over the whole sequence.  DC / SC: an entry that sees nothing, one in which about 300 rows see keys, one in which every
    row does."""
    for cid in ("DA", "SA"):
        lo, hi = M.definition_bounds(M.BY_ID[cid])
        S = M.BY_ID[cid].Sq
        i = np.arange(S)
        assert any((l == 0).all() and (h == i + 1).all() for l, h in zip(lo, hi)), cid
        if cid == "DA":                                                # a document of about 1500 positions that is not the sequence
            assert any((((h - l) >= 1400) & (l > 0)).any() for l, h in zip(lo, hi)), cid
        else:                                                          # a span of about 1500 positions that is not the sequence
            assert any(((h - i - 1) >= 1400).any() and not (h == S).all() for l, h in zip(lo, hi)), cid
    lo, hi = M.definition_bounds(M.BY_ID["SA"])
    assert any((l == 0).all() and (h == 2048).all() for l, h in zip(lo, hi))
    for cid in ("DC", "SC", "DC8", "SC8"):
        lo, hi = M.definition_bounds(M.BY_ID[cid])
        seeing = [(l < h).sum() for l, h in zip(lo, hi)]
        assert 0 in seeing and 300 in seeing and M.BY_ID[cid].Sq in seeing, (cid, seeing)


def _launches(case):
    """(what, n_items, slots, n_inner, decode id -> (batch entry, first unit, units, "rows" | "keys")) of the case's flash launches
    at 256 CUs."""
    c = case
    fk, fn, fslots, f_inner = M.fwd_launch(c)
    rows = 128 if fk == "fwd_wave4" else 256
    ks = max(1, c.k_splits)

    def fwd_item(w):
        t = (w // ks) % (f_inner // ks)
        t = (f_inner // ks - 1 - t) if c.causal else t
        return w // f_inner // c.Hq, t * rows, rows, "rows"
    out = [(fk, fn, fslots, f_inner, fwd_item)]
    if c.bwd:
        _, qn, qslots, nblk = M.dq_launch(c)

        def dq_item(w):
            t = w % nblk
            t = (nblk - 1 - t) if c.causal else t
            return w // nblk // c.Hq, t * 256, 256, "rows"
        _, kn, kslots, kblk = M.dkdv_launch(c)
        slabs = (c.Hq // c.Hkv) // c.gsub

        def dkdv_item(w):
            return w // kblk // slabs // c.Hkv, (w % kblk) * 128, 128, "keys"
        out += [("dq_wave8", qn, qslots, nblk, dq_item), ("dkdv_wave8", kn, kslots, kblk, dkdv_item)]
    return out


def _wg_lists(L, n_items, slots, n_inner):
    """The decoded ids every workgroup of a persistent launch serves, in order (usp_common.hpp: ItemWalk::at, ::dealt)."""
    by_xcd = slots % 8 == 0 and n_items % 8 == 0
    items_l = n_items // 8 if by_xcd else n_items
    wgs_l = slots // 8 if by_xcd else slots
    lists = []
    for x in range(8 if by_xcd else 1):
        for wg in range(wgs_l):
            ids, p = [], 0
            while True:
                loc = p * wgs_l + ((wgs_l - 1 - wg) if p & 1 else wg)
                if loc >= items_l:
                    break
                ids.append(L.usp_deal_item(x * items_l + loc, n_inner, items_l))
                p += 1
            lists.append(ids)
    return lists


def test_table_reaches_the_item_walks_and_is_multi_pass(walk_lib):
    seen = {"doc": set(), "span": set(), "sink": set()}
    for c in M.CASES:
        for kind, n, slots, n_inner, _ in _launches(c):
            assert n > slots, (c.id, kind, n, slots)                            # multi-pass
            ids, items_l, dealt, _ = _walk(walk_lib, n, slots, n_inner, 1, False)
            assert sorted(ids) == list(range(n)), (c.id, kind)                  # every item exactly once
            assert sorted(i for l in _wg_lists(walk_lib, n, slots, n_inner) for i in l) == list(range(n)), (c.id, kind)
            by_xcd = slots % 8 == 0 and n % 8 == 0
            if by_xcd and items_l >= n_inner:
                seen[c.family].add("XCD runs with whole heads")
            if dealt:
                seen[c.family].add("regular dealing" if n_inner % items_l == 0 else "irregular dealing")
            if n % 8:
                seen[c.family].add("count not divisible by 8")
    print(f"[large-masks-walks] {seen}")
    for fam in ("doc", "span"):
        assert {"XCD runs with whole heads", "count not divisible by 8"} <= seen[fam], (fam, seen[fam])
        assert seen[fam] & {"regular dealing", "irregular dealing"}, (fam, seen[fam])
    assert {"regular dealing", "irregular dealing"} <= seen["doc"] | seen["span"], seen
    assert [c.id for c in M.CASES] == ["DA", "DB", "DC", "LD", "SA", "SB", "SC", "LS", "KA", "KA2", "KAw", "KB", "KE", "DC8", "SC8"]


@pytest.mark.parametrize("cid", ["DC", "SC", "DC8", "SC8"])
def test_workgroups_go_live_empty_live(walk_lib, cid):
    """Whether an item streams zero tiles is decided from the definition's masks: a forward or dQ item is empty iff none of its rows
    sees a key, a dK/dV item iff none of its keys is seen."""
    c = M.BY_ID[cid]
    lo, hi = M.definition_bounds(c)
    row_sees = lo < hi
    key_sees = np.stack([np.less(*IR.key_bounds(l, h, c.Sk)) for l, h in zip(lo, hi)])
    for kind, n, slots, n_inner, item in _launches(c):
        def empty(w):
            b, first, units, side = item(w)
            return not (row_sees if side == "rows" else key_sees)[b, first:first + units].any()
        steps = {(empty(a), empty(b)) for ids in _wg_lists(walk_lib, n, slots, n_inner) for a, b in zip(ids[:-1], ids[1:])}
        n_empty = sum(empty(w) for w in range(n))
        print(f"[large-masks-walks] {cid} {kind}: {n} items, {n_empty} empty, steps (empty, empty) seen {sorted(steps)}")
        assert (True, False) in steps and (False, True) in steps, (cid, kind, steps)


# ---- 3. the comparisons can fail ----------------------------------------------------------------------------------------------
MUTANT_ENTRY = {"DA": 0, "SA": 0, "DC": 3, "SC": 4}                   # the batch entry whose list is mutated (KV group 0)


def _list_mutants(case, b):
    """[(name, (cu, spans))]: every boundary of the entry's document list moved by one position each way (onto its neighbour: the two
    documents merge), every span start and end moved by one each way where the list stays valid."""
    cu, sp = M.entries(case)[b]
    S = case.S_total
    out = []
    for i in range(1, len(cu or []) - 1):
        for move in (-1, 1):
            e = cu[i]
            mut = [x for x in cu if x != e] if not (cu[i - 1] < e + move < cu[i + 1]) else [e + move if x == e else x for x in cu]
            spans = sp
            if not isinstance(sp, str):                                # spans must stay inside one document of the moved list
                st = doc_ref.starts(mut, S)
                if any(st[s] != st[e_ - 1] for s, e_ in sp):
                    continue
            out.append((f"boundary {e} {move:+d}", (mut, spans)))
    if not isinstance(sp, str):
        st = doc_ref.starts(cu or [0, S], S)
        for n, (s, e) in enumerate(sp):
            for ds, de in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                s2, e2 = s + ds, e + de
                prev_e = sp[n - 1][1] if n else 0
                next_s = sp[n + 1][0] if n + 1 < len(sp) else S
                if not (prev_e <= s2 < e2 <= next_s) or st[s2] != st[e2 - 1]:
                    continue
                out.append((f"span ({s}, {e}) -> ({s2}, {e2})", (cu, [x if m != n else (s2, e2) for m, x in enumerate(sp)])))
    return out


def _rows_that_differ(a, b):
    ca, cb = M._canon(*a), M._canon(*b)
    return np.nonzero((ca[0] != cb[0]) | (ca[1] != cb[1]))[0]


@pytest.mark.parametrize("cid", ["DA", "SA", "DC", "SC"])
def test_mutants_fail(cid):
    c = M.BY_ID[cid]
    b, G, scale = MUTANT_ENTRY[cid], c.Hq // c.Hkv, c.D ** -0.5
    nd = M.inputs(c)
    dt = getattr(torch, c.dt)
    q, k, v, do = (torch.from_numpy(x[b:b + 1, :, :n]).to(dt) for x, n in ((nd.q, G), (nd.k, 1), (nd.v, 1), (nd.do, G)))
    lo_all, hi_all = M.definition_bounds(c)
    lo, hi = lo_all[b], hi_all[b]
    ro, rl = IR.ref_fwd(q, k, v, scale, lo, hi)
    o16 = ro.to(dt)
    dq, dk, dv, _ = IR.ref_bwd(do, q, k, v, o16, rl, scale, lo, hi)
    true = dict(out=ro, lse=rl, dq=dq, dk=dk, dv=dv)

    def by_rows(lo_m, hi_m, rows, backward_too=True):
        """What the GPU test would see of kernels that read (lo_m, hi_m) on `rows` (a range): the forward's out / lse, and -- from the
        exact lse and delta the test hands the backward -- dq of those rows and their share of dk / dv."""
        r = slice(int(rows[0]), int(rows[-1]) + 1)
        got = {n: t.clone() for n, t in true.items()}
        got["out"][:, r], got["lse"][:, :, r] = IR.ref_fwd(q[:, r], k, v, scale, lo_m[r], hi_m[r])
        m_ = IR.ref_bwd(do[:, r], q[:, r], k, v, o16[:, r], rl[:, :, r], scale, lo_m[r], hi_m[r])
        got["dq"][:, r] = m_[0]
        if backward_too:
            t_ = IR.ref_bwd(do[:, r], q[:, r], k, v, o16[:, r], rl[:, :, r], scale, lo[r], hi[r])
            got["dk"] += m_[1] - t_[1]
            got["dv"] += m_[2] - t_[2]
        return got

    def by_keys(blk):
        """dk / dv of the 128-key block `blk` from the key bounds of the block before it (the dK/dV launch reads the key arrays)."""
        klo, khi = IR.key_bounds(lo, hi, c.Sk)
        own0, n = blk * 128, min(128, c.Sk - blk * 128)
        klo_m, khi_m = klo[own0 - 128:own0 - 128 + n], khi[own0 - 128:own0 - 128 + n]
        i = np.arange(c.Sq, dtype=np.int64)
        lo_m = own0 + np.searchsorted(khi_m, i, side="right")         # keys of the block with key_hi <= i: hidden from row i
        hi_m = own0 + np.searchsorted(klo_m, i, side="right")         # keys of the block with key_lo <= i
        t_lo, t_hi = np.clip(lo, own0, own0 + n), np.clip(hi, own0, own0 + n)
        rows = _rows_that_differ((lo_m, hi_m), (t_lo, t_hi))
        if not len(rows):
            return None, rows, (lo_m, hi_m)
        ks = slice(own0, own0 + n)
        m_ = IR.ref_bwd(do, q, k[:, ks], v[:, ks], o16, rl, scale, lo_m - own0, hi_m - own0)
        got = {n_: t.clone() for n_, t in true.items()}
        got["dk"][:, ks], got["dv"][:, ks] = m_[1], m_[2]
        return got, rows, (lo_m, hi_m)

    cands = []                                                         # (name, thunk -> (got | None, rows that differ, bounds))
    for name, lists in _list_mutants(c, b):
        all_lists = list(M.entries(c))
        all_lists[b] = lists
        cands.append((name, M.definition_bounds(c, all_lists[b:b + 1]), "rows"))
    other = (b + 1) % c.B
    cands.append((f"the arrays of entry {other} for entry {b}", (lo_all[other:other + 1], hi_all[other:other + 1]), "rows"))
    for t in range(1, -(-c.Sq // 256)):
        lo_m, hi_m = lo.copy(), hi.copy()
        n = min(256, c.Sq - t * 256)
        lo_m[t * 256:t * 256 + n], hi_m[t * 256:t * 256 + n] = lo[(t - 1) * 256:(t - 1) * 256 + n], hi[(t - 1) * 256:(t - 1) * 256 + n]
        cands.append((f"query tile {t} with the bounds of tile {t - 1}", (lo_m[None], hi_m[None]), "tile"))
    for blk in range(1, -(-c.Sk // 128)):
        cands.append((f"key block {blk} with the bounds of block {blk - 1}", blk, "keys"))

    judged = dropped = undetected = 0
    exceptions = []
    for name, m, side in cands:
        if side == "keys":
            got, rows, (lo_m, hi_m) = by_keys(m)
            t_lo, t_hi = np.clip(lo, m * 128, m * 128 + 128), np.clip(hi, m * 128, m * 128 + 128)
        else:
            lo_m, hi_m = m[0][0], m[1][0]
            rows = _rows_that_differ((lo_m, hi_m), (lo, hi))
            got = by_rows(lo_m, hi_m, rows, side == "rows") if len(rows) else None
            t_lo, t_hi = lo, hi
        if got is None:
            dropped += 1
            continue
        judged += 1
        ver = NI.verdicts(got, true, c.dt, c.Sq, c.Sk, G)
        if all(ok for ok, _ in ver.values()):
            seen = np.minimum(np.maximum(hi_m - lo_m, 0), np.maximum(t_hi - t_lo, 0))[rows]
            if (seen <= 1).all():                                      # the project's known exception: P = 1, dS = 0 by arithmetic
                exceptions.append(name)
            else:
                undetected += 1
                print(f"[large-masks-mutants] {cid}: UNDETECTED {name}: " + " ".join(f"{n}={r:.2f}" for n, (_, r) in ver.items()))
    print(f"[large-masks-mutants] {cid} entry {b}, KV group 0: judged {judged} / dropped, mask unchanged {dropped} / exceptions "
          f"(the changed rows see a single key) {len(exceptions)} {exceptions} / undetected {undetected}")
    assert judged >= 8 and undetected == 0 and 20 * len(exceptions) <= judged, (cid, judged, undetected, exceptions)
