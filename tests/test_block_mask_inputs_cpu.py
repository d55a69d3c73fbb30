"""The block-sparse edge tests without a GPU: what tests/block_mask_inputs.py claims about its tables, block_mask_ref.enumerate_lists
pinned against a brute-force enumeration from block_mask_ref.visible, and mutants in fp64 -- attention computed FROM LISTS, the way
the kernels walk them, with a fault planted in the lists -- that must fail needle_inputs.verdicts at >= 2 x the bound on the LONG
S = 4400 needle inputs (and mostly do not on white noise, which is why the long-list cases use needles)."""
import numpy as np
import pytest
import torch

import block_mask_inputs as BI
import block_mask_ref as R
import needle_inputs as NI

BAR = 2.0           # a mutant must miss the bound by this factor: the kernels' honest rounding reaches 0.49 of it
                    # (profiles/large_launch_masks.txt), so a fault at 2 x still fails with that error against it


# ---- 1. enumerate_lists against a brute-force enumeration ------------------------------------------------------------------------
def brute_lists(m4, S, causal):
    """A 64-wide tile is listed iff its block is live -- under causal: iff any (row, key) pair of the block is visible -- and the
    tile exists; from block_mask_ref.visible alone."""
    B, Hq, nb, _ = m4.shape
    t4 = torch.from_numpy(m4)
    pad = nb * 128 - S
    fwd, dq, dkdv = {}, {}, {}
    tiles = lambda c: [t for t in (2 * c, 2 * c + 1) if 64 * t < S]
    for b in range(B):
        vis = R.visible(t4, b, 0, S, S, causal)                                            # (Hq, S, S)
        vis = torch.nn.functional.pad(vis, (0, pad, 0, pad))
        blk = vis.reshape(Hq, nb, 128, nb, 128).permute(0, 1, 3, 2, 4).reshape(Hq, nb, nb, -1).any(-1).numpy()
        for h in range(Hq):
            for r in range(nb):
                fwd[b, h, r] = [t for c in range(nb) if blk[h, r, c] for t in tiles(c)]
                dkdv[b, h, r] = [t for rr in range(nb) if blk[h, rr, r] for t in tiles(rr)]
            for i in range((nb + 1) // 2):
                ent = []
                for c in range(nb):
                    bits = int(blk[h, 2 * i, c]) + (2 * int(blk[h, 2 * i + 1, c]) if 2 * i + 1 < nb else 0)
                    ent += [4 * t + bits for t in tiles(c)] if bits else []
                dq[b, h, i] = ent
    return dict(fwd=fwd, dq=dq, dkdv=dkdv)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("S", BI.RAGGED_S + (4400,))
def test_enumerate_lists_is_the_brute_force_enumeration(S, causal):
    nb = R.n_blocks(S)
    for kind in ("all", "random", "last_only", "holes"):
        m = BI.ragged_mask(kind, 1 if S == 4400 else 2, 2, S)
        got, want = R.enumerate_lists(m, S, causal), brute_lists(m, S, causal)
        assert got == want, (S, causal, kind)
        if kind == "all" and BI.one_tile_last_block(S):          # the one-tile last block, counted in all three families
            assert len(got["fwd"][0, 0, nb - 1]) == 2 * nb - 1 and got["fwd"][0, 0, nb - 1][-1] == 2 * (nb - 1)
            assert len(got["dq"][0, 0, (nb - 1) // 2]) == 2 * nb - 1 and got["dq"][0, 0, (nb - 1) // 2][-1] // 4 == 2 * (nb - 1)
            assert len(got["dkdv"][0, 0, nb - 1]) == (1 if causal else 2 * nb - 1) and got["dkdv"][0, 0, nb - 1][-1] == 2 * (nb - 1)
            assert len(got["dkdv"][0, 0, 0]) == 2 * nb - 1


def test_which_sizes_have_a_one_tile_last_block():
    assert [S for S in BI.RAGGED_S + (4400, 8300, 333) if BI.one_tile_last_block(S)] == [64, 257, 300, 320, 4400]


# ---- 2. what the tables claim ----------------------------------------------------------------------------------------------------
def test_ragged_table():
    assert len(BI.RAGGED) == 160
    for S in BI.RAGGED_S:
        assert {(c.Hq, c.Hkv, c.D) for c in BI.RAGGED if c.S == S} == set(BI.SHAPES3)
    for causal in (True, False):             # last_only: every non-empty list ends in, or consists of, the short block
        lists = R.enumerate_lists(BI.ragged_mask("last_only", 1, 2, 300), 300, causal)
        for fam, d in lists.items():
            for ent in d.values():
                assert not ent or (ent[-1] // 4 if fam == "dq" else ent[-1]) == 4, (fam, ent)


def test_long_table_list_lengths():
    """S = 4400: the counts 63, 64, 65 and 66 each occur in every family over the three circulant widths.  (S = 8300 has a
    two-tile last block, so its circulant lists are even: 62 ... 68.)  Every `dense` case has a list of >= 65 entries in every
    family, >= 129 at S = 8300 (asserted in long_build)."""
    for S, Hq, Hkv, D, dt in BI.LONG_SHAPES:
        seen = {"fwd": set(), "dq": set(), "dkdv": set()}
        for c in BI.LONG:
            if (c.S, c.D) == (S, D):
                b = BI.long_build(c)
                if c.kind.startswith("circ"):
                    for fam in seen:
                        seen[fam] |= set(b.lens[fam])
        for fam, s in seen.items():
            assert s >= ({63, 64, 65, 66} if S == 4400 else {64, 66}), (S, fam, sorted(s))
        print(f"[bsp-edges-cpu] S{S} circulant list lengths: " + " ".join(f"{f}={sorted(s)}" for f, s in seen.items()))


@pytest.mark.parametrize("c", BI.LONG, ids=lambda c: c.id)
def test_long_needle_conditions(c):
    b = BI.long_build(c)
    res = BI.long_needle_conditions(c, b)
    pos = {(fam, p) for fam, _, _, p, _, _ in b.info.records}
    for fam in ("fwd", "dkdv"):              # edge needles at the positions 0 and last of both families, and 63 / 64 / 65 where the lists reach
        assert (fam, 0) in pos and any(p >= 60 for f, p in pos if f == fam), (c.id, sorted(pos))
        if c.kind in ("dense", "circ33"):
            assert {(fam, 63), (fam, 64), (fam, 65)} <= pos, (c.id, sorted(pos))
    print(f"[bsp-edges-cpu] {c.id}: needle mass >= {min(r[0] for r in res):.4f}, {len(b.edges)} edge needles")


def test_heads_table():
    for c in BI.HEADS:
        m, slots = BI.heads_mask(c.Hq, c.Hkv, c.causal)          # (asserts the patterns from enumerate_lists)
        for hk in range(c.Hkv):
            assert sorted(p for (b, k_, kb), p in slots.items() if k_ == hk) == sorted(BI.HEAD_PATTERNS)
        assert BI.divisors_with_zero(c.G) == ([0, 1, 2, 4] if c.G == 4 else [0, 1, 3])


def test_fuzz_coverage_floor():
    """Over the default 24 seeds: 14 cases with S mod 128 in (0, 64], 4 with a non-contiguous mask, 14 with G >= 3 and
    dkdv_heads < G (the floors: 4, 3, 3)."""
    cov = BI.fuzz_coverage()
    print(f"[bsp-edges-cpu] fuzz coverage of the first {BI.FUZZ_DEFAULT} seeds: {cov}")
    assert cov == dict(one_tile_last_block=14, non_contiguous_mask=4, head_walk_split=14)
    assert cov["one_tile_last_block"] >= 4 and cov["non_contiguous_mask"] >= 3 and cov["head_walk_split"] >= 3
    for seed in range(BI.FUZZ_DEFAULT):
        c = BI.fuzz_case(seed)
        assert 1 <= c.S <= 700 and c.G % c.heads == 0 and c.m4.shape == (c.B, c.Hq, R.n_blocks(c.S), R.n_blocks(c.S))


# ---- 3. attention from lists, and mutants of the lists ---------------------------------------------------------------------------
class ListModel:
    """fp64 attention of batch entry 0 computed from lists as the kernels walk them: the forward of row block r over the 64-key
    tiles of its list, dQ of a pair of row blocks over its entries and their half bits, dK / dV of key block c over the 64-row tiles
    of its transposed list; a tile that occurs twice counts twice.  The backward takes lse and delta as given.  Results are kept per
    (family, head, block, entries), so a mutant recomputes only the lists it changed."""

    def __init__(self, q, k, v, do, causal):
        self.q, self.k, self.v, self.do = (torch.from_numpy(np.asarray(x[0], dtype=np.float64)) for x in (q, k, v, do))
        self.S, self.Hq, self.D = self.q.shape
        self.Hkv = self.k.shape[1]
        self.G, self.causal, self.scale = self.Hq // self.Hkv, causal, self.D ** -0.5
        self.memo = {}

    def _idx(self, tiles):
        idx = (torch.tensor(tiles, dtype=torch.int64)[:, None] * 64 + torch.arange(64)[None, :]).reshape(-1)
        return idx.clamp(max=self.S - 1), idx < self.S, idx

    def _fwd(self, h, r, ent):
        rows = torch.arange(128 * r, min(self.S, 128 * r + 128))
        out, lse = torch.zeros(len(rows), self.D, dtype=torch.float64), torch.full((len(rows),), float("-inf"), dtype=torch.float64)
        if ent:
            at, valid, idx = self._idx(ent)
            s = self.q[rows, h] @ self.k[at, h // self.G].T * self.scale
            vis = valid[None, :] & ((idx[None, :] <= rows[:, None]) if self.causal else torch.ones_like(s, dtype=torch.bool))
            s = s.masked_fill(~vis, float("-inf"))
            m = s.amax(-1, keepdim=True)
            m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
            p = torch.exp(s - m)
            l = p.sum(-1, keepdim=True)
            live = l[:, 0] > 0
            lse[live] = (m + torch.log(l))[live, 0]
            out[live] = (p / l)[live] @ self.v[at, h // self.G]
        return out, lse

    def _p_ds(self, rows_at, keys_at, vis, h, lse, delta):
        s = self.q[rows_at, h] @ self.k[keys_at, h // self.G].T * self.scale
        l = lse[h, rows_at][:, None]
        fin = torch.isfinite(l)
        p = torch.where(vis & fin, torch.exp(s - torch.where(fin, l, torch.zeros_like(l))), torch.zeros_like(s))
        ds = p * (self.do[rows_at, h] @ self.v[keys_at, h // self.G].T - delta[h, rows_at][:, None]) * self.scale
        return p, ds

    def _dq(self, h, i, ent, lse, delta):
        rows = torch.arange(256 * i, min(self.S, 256 * i + 256))
        if not ent:
            return torch.zeros(len(rows), self.D, dtype=torch.float64)
        at, valid, idx = self._idx([e // 4 for e in ent])
        bits = torch.tensor([e & 3 for e in ent], dtype=torch.int64).repeat_interleave(64)
        half = (rows // 128 - 2 * i)[:, None]
        vis = ((bits[None, :] >> half) & 1).bool() & valid[None, :]
        if self.causal:
            vis = vis & (idx[None, :] <= rows[:, None])
        _, ds = self._p_ds(rows, at, vis, h, lse, delta)
        return ds @ self.k[at, h // self.G]

    def _dkdv(self, h, c, ent, lse, delta):
        keys = torch.arange(128 * c, min(self.S, 128 * c + 128))
        if not ent:
            z = torch.zeros(len(keys), self.D, dtype=torch.float64)
            return z, z
        at, valid, idx = self._idx(ent)
        vis = valid[:, None] & ((keys[None, :] <= idx[:, None]) if self.causal else torch.ones(len(at), len(keys), dtype=torch.bool))
        p, ds = self._p_ds(at, keys, vis, h, lse, delta)
        return ds.T @ self.q[at, h], p.T @ self.do[at, h]

    def _get(self, fam, h, blk, ent, fn, *a):
        key = (fam, h, blk, tuple(ent))
        if key not in self.memo:
            self.memo[key] = fn(h, blk, ent, *a)
        return self.memo[key]

    def forward(self, lists):
        out = torch.zeros(1, self.S, self.Hq, self.D, dtype=torch.float64)
        lse = torch.zeros(1, self.Hq, self.S, dtype=torch.float64)
        for (b, h, r), ent in lists["fwd"].items():
            o, l = self._get("fwd", h, r, ent, self._fwd)
            out[0, 128 * r:128 * r + 128, h], lse[0, h, 128 * r:128 * r + 128] = o, l
        return out, lse

    def backward(self, lists, out, lse):
        """(dq, dk, dv) under `lists`, lse as given and delta from `out` (what the true forward hands the backward)."""
        delta = (self.do * out[0]).sum(-1).T                                              # (Hq, S)
        dq = torch.zeros(1, self.S, self.Hq, self.D, dtype=torch.float64)
        dk = torch.zeros(1, self.S, self.Hkv, self.D, dtype=torch.float64)
        dv = torch.zeros_like(dk)
        for (b, h, i), ent in lists["dq"].items():
            dq[0, 256 * i:256 * i + 256, h] = self._get("dq", h, i, ent, self._dq, lse[0], delta)
        for (b, h, c), ent in lists["dkdv"].items():
            a, b_ = self._get("dkdv", h, c, ent, self._dkdv, lse[0], delta)
            dk[0, 128 * c:128 * c + 128, h // self.G] += a
            dv[0, 128 * c:128 * c + 128, h // self.G] += b_
        return dq, dk, dv

    def run(self, lists, truth=None):
        out, lse = self.forward(lists)
        fo, fl = (out, lse) if truth is None else (truth["out"], truth["lse"])
        return dict(zip(("out", "lse", "dq", "dk", "dv"), (out, lse) + self.backward(lists, fo, fl)))


def _map(lists, fn):
    return {fam: {key: fn(fam, ent) for key, ent in d.items()} for fam, d in lists.items()}


def mutants(c, built):
    """name -> (mutated lists, the tensors the fault touches).  LAST: the one tile of the last block (S = 4400: tile 68)."""
    true, m4 = built.lists, built.m4
    LAST = 2 * (m4.shape[-1] - 1)
    tile = lambda fam, e: e // 4 if fam == "dq" else e
    every = ("out", "lse", "dq", "dk", "dv")
    res = {}
    for name, (h, r, kb, pos) in BI.lost_block_mutations(c, built).items():
        if name != "last":
            m = m4.copy()
            m[0, h, r, kb] = False
            res[f"one block lost at {'dQ' if name == 'fwd' else 'transposed'} list position {pos}"] = (R.enumerate_lists(m, c.S, c.causal), every)
    res["dQ entries 64.. read as entries 0.. (stale refill)"] = (
        dict(true, dq={key: e[:64] + e[:max(0, len(e) - 64)] for key, e in true["dq"].items()}), ("dq",))
    res["lists truncated at 64"] = (_map(true, lambda fam, e: e[:64]), every)
    res["the last, one-tile entry lost"] = (_map(true, lambda fam, e: e[:-1] if e and tile(fam, e[-1]) == LAST else e), every)
    res["the last block given a second tile (clamped onto the last: counted twice)"] = (
        _map(true, lambda fam, e: e + e[-1:] if e and tile(fam, e[-1]) == LAST else e), every)
    res["transposed lists from the untransposed mask"] = (
        dict(true, dkdv=R.enumerate_lists(np.ascontiguousarray(m4.swapaxes(-1, -2)), c.S, c.causal)["dkdv"]), ("dk", "dv"))
    return res


MUTANT_CASES = [c for c in BI.LONG if c.S == 4400 and c.kind == "dense" and (c.D == 64 or not c.causal)]


@pytest.mark.parametrize("c", MUTANT_CASES, ids=lambda c: c.id)
def test_list_mutants_fail_on_needles_and_mostly_pass_on_white_noise(c):
    """At the LONG S = 4400 `dense` inputs (D = 64: causal and full; D = 128: full): attention from the TRUE lists is the reference
    (block_mask_ref.ref_all, to 1e-9) and passes needle_inputs.verdicts; every mutant misses the bound by >= 2 x in every tensor
    its fault touches.  The same mutants on white noise are printed; at the bf16 tolerances the one-lost-block mutant passes at least one gradient there."""
    built = BI.long_build(c)
    counted = 0
    for white in (False, True):
        nd = BI.long_build(c, white=white).nd
        model = ListModel(nd.q, nd.k, nd.v, nd.do, c.causal)
        truth = model.run(built.lists)
        if not white:                         # the list walk is the reference
            t64 = [torch.from_numpy(np.asarray(x, dtype=np.float64)) for x in (nd.do, nd.q, nd.k, nd.v)]
            ref = R.ref_all(*t64, c.D ** -0.5, torch.from_numpy(np.array(built.mask)), c.causal)
            for n, r_ in zip(("out", "lse", "dq", "dk", "dv"), ref):
                assert float((truth[n] - r_).abs().max()) < 1e-9, (c.id, n)
        verdict = NI.verdicts(truth, truth, c.dt, c.S, c.S, c.G)
        assert all(ok for ok, _ in verdict.values())
        counted += 1
        for name, (lists, touched) in mutants(c, built).items():
            got = model.run(lists, truth)
            verdict = NI.verdicts({n: got[n] for n in touched}, truth, c.dt, c.S, c.S, c.G)
            print(f"[bsp-edges-cpu] {c.id} {'white noise' if white else 'needles'}: {name}: " +
                  " ".join(f"{n}={verdict[n][1]:.2f}" for n in touched))
            if not white:
                for n in touched:
                    assert verdict[n][1] >= BAR, f"{c.id}: mutant `{name}` reaches only {verdict[n][1]:.2f} x the bound in {n}"
                counted += 1
            elif name.startswith("one block lost at dQ") and c.dt == "bfloat16":
                # (at the fp16 tolerances, five times tighter, white noise does see the block: 1.4 ... 1.9 x in the gradients of the
                # causal D = 64 case, still under the 2 x bar the needles clear by a factor of seven)
                assert any(verdict[n][0] for n in ("dq", "dk", "dv")), (c.id, name, verdict)
    assert counted == 2 + 7
