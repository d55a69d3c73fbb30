"""Proof that needle inputs (tests/needle_inputs.py) have power where N(0,1) inputs have none.

A small fp64 attention with a pluggable mutation stands in for a subtly wrong kernel: for ONE 256-row query tile (or one
dK/dV item) it may weight keys 0x or 2x, read K or V through an index map, or use another mask.  Forward mutants run the
plain forward; backward mutants follow the block contract of the GPU files (exact lse, delta from the 16-bit-rounded exact
out) with the mutated operands.  Its unmutated form agrees with tests/attn_ref_torch.py to 1e-10.

Every mutant must FAIL `needle_inputs.verdicts` -- the function tests/test_gpu_needle.py asserts with: golden_util's
comparator, TOL, lse 2e-3 + 1e-4 |lse|, long_sum_atol -- in every tensor it corrupts, with the worst error at least 3x its
bound (honest 16-bit noise is <= 1x by the definition of TOL).  And as the record of why this file exists: the drop /
twice / mispair mutants at S = 32768 on N(0,1) inputs pass.  SURVEY.md section 8(c) holds the measured table
(`python tests/test_needle_cpu.py` prints it).
"""
import numpy as np
import pytest
import torch

import needle_inputs as NI
from attn_ref_torch import ref_bwd, ref_fwd
from golden_util import TOL, close_mask, round_to

QT = 256            # rows of a forward / dQ work item
MARGIN = 3.0


class Mask:
    """Visibility of key j to row i: causal (bottom-right), window, packed sequences (causal inside each), with optional
    off-by-one shifts for the mutants."""

    def __init__(self, Sq, Sk, causal=False, window=None, seqs=None, shift=0):
        self.Sq, self.Sk, self.causal, self.window, self.seqs, self.shift = Sq, Sk, causal, window, seqs, int(shift or 0)

    def vis(self, r0, r1, d_right=0, d_left=0, d_first=0, d_half=0, shift_right=None, shift_left=None):
        """`shift_right` / `shift_left`: the shift one bound is computed with, in place of the mask's own (the mutants that
        move one bound only, or the wrong way)."""
        i = torch.arange(r0, r1)[:, None]
        j = torch.arange(self.Sk)[None, :]
        if self.seqs is not None:                        # (first, len) per sequence, same table for rows and keys
            v = torch.zeros(r1 - r0, self.Sk, dtype=torch.bool)
            for s0, n in self.seqs:
                rows = (i >= s0) & (i < s0 + n)
                keys = (j >= s0 + d_first) & (j <= i + d_right)
                if d_half:                               # the ring's half boundary: rows of the second half and the keys
                    h = s0 + n // 2                      # of the first half meet in a block of their own
                    second = i >= h
                    if d_half < 0:
                        keys = keys & ~(second & (j == h - 1))
                v |= rows & keys
            return v
        left, right = (-1, -1) if self.window is None else self.window
        if self.causal:
            right = 0
        off = self.Sk - self.Sq
        sr = self.shift if shift_right is None else shift_right
        sl = self.shift if shift_left is None else shift_left
        v = torch.ones(r1 - r0, self.Sk, dtype=torch.bool)
        if right >= 0:
            v &= j <= i + off + sr + right + d_right
        if left >= 0:
            v &= j >= i + off + sl - left + d_left
        return v


def tile_fwd_bwd(T, h, r0, r1, mask, scale, mut=None, lse=None, delta=None):
    """Rows [r0, r1) of query head h (tensors of one batch entry: q, do (Sq,Hq,D), k, v (Sk,Hkv,D), fp64) -> out, lse of
    the rows and, given exact `lse` / `delta` (Hq,Sq), dq of the rows and the rows' contributions to dk, dv (Sk,D).
    `mut`: dict(mult=(k0, k1, m), kmap=idx, vmap=idx, vis=dict(kwargs of Mask.vis), head=h2)."""
    mut = mut or {}
    G = T["q"].shape[1] // T["k"].shape[1]
    hs = mut.get("head", h)                              # the head whose rows this item reads
    q, do = T["q"][r0:r1, hs], T["do"][r0:r1, hs]
    k, v = T["k"][:, h // G], T["v"][:, h // G]
    kmap = mut.get("kmap")
    vmap = mut.get("vmap")
    km = k if kmap is None else k[kmap]
    vm = v if vmap is None else v[vmap]
    vis = mask.vis(r0, r1, **mut.get("vis", {}))
    s = (q @ km.T) * scale
    s = s.masked_fill(~vis, float("-inf"))
    w = torch.ones(s.shape[1], dtype=torch.float64)
    if "mult" in mut:
        k0, k1, m = mut["mult"]
        w[k0:k1] = m
    if "dup" in mut:                                     # key counted once more for the rows that must not double it
        w[mut["dup"]] = 2.0
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    p = torch.exp(s - mx) * w
    l = p.sum(-1, keepdim=True)
    ok = l > 0
    out = torch.where(ok, (p / torch.where(ok, l, torch.ones_like(l))) @ vm, torch.zeros_like(q))
    lse_rows = torch.where(ok[:, 0], (mx + torch.log(torch.where(ok, l, torch.ones_like(l))))[:, 0],
                           torch.full_like(l[:, 0], float("-inf")))
    if lse is None:
        return out, lse_rows
    L, dl = lse[hs, r0:r1, None], delta[hs, r0:r1, None]
    fin = torch.isfinite(L)
    P = torch.where(fin, torch.exp(s - torch.where(fin, L, torch.zeros_like(L))), torch.zeros_like(s)) * w
    dS = P * (do @ vm.T - dl) * scale
    dq = dS @ km
    dk = torch.zeros_like(k)
    dv = torch.zeros_like(v)
    dk.index_add_(0, torch.arange(k.shape[0]) if kmap is None else kmap, dS.T @ q)
    dv.index_add_(0, torch.arange(v.shape[0]) if vmap is None else vmap, P.T @ do)
    return out, lse_rows, dq, dk, dv


class Exact:
    """The unmutated fp64 result of one batch entry, tile by tile, and the same with one item mutated."""

    def __init__(self, q, k, v, do, dt, mask, scale):
        self.T = {n: torch.from_numpy(np.asarray(x, dtype=np.float64)) for n, x in (("q", q), ("k", k), ("v", v), ("do", do))}
        self.dt, self.mask, self.scale = dt, mask, scale
        Sq, Hq, D = self.T["q"].shape
        Sk, Hkv, _ = self.T["k"].shape
        self.G = Hq // Hkv
        self.out = torch.zeros(Sq, Hq, D, dtype=torch.float64)
        self.lse = torch.zeros(Hq, Sq, dtype=torch.float64)
        for h in range(Hq):
            for r0 in range(0, Sq, QT):
                r1 = min(Sq, r0 + QT)
                self.out[r0:r1, h], self.lse[h, r0:r1] = tile_fwd_bwd(self.T, h, r0, r1, mask, scale)
        o16 = torch.from_numpy(round_to(self.out.numpy().astype(np.float32), dt).astype(np.float64))
        self.delta = (self.T["do"] * o16).sum(-1).T.contiguous()
        self.dq = torch.zeros_like(self.out)
        self.dk = torch.zeros(Sk, Hkv, D, dtype=torch.float64)
        self.dv = torch.zeros_like(self.dk)
        for h in range(Hq):
            for r0 in range(0, Sq, QT):
                r1 = min(Sq, r0 + QT)
                _, _, self.dq[r0:r1, h], dk, dv = self._tile(h, r0, r1)
                self.dk[:, h // self.G] += dk
                self.dv[:, h // self.G] += dv

    def _tile(self, h, r0, r1, mut=None):
        return tile_fwd_bwd(self.T, h, r0, r1, self.mask, self.scale, mut, self.lse, self.delta)

    def want(self):
        return dict(out=self.out, lse=self.lse, dq=self.dq, dk=self.dk, dv=self.dv)

    def mutated(self, h, r0, r1, mut, keys=None):
        """The result with rows [r0, r1) of head h computed under `mut`.  `keys` = (k0, k1): a dK/dV item -- only the dk /
        dv rows of that key block take the mutated contributions (out, lse, dq stay exact)."""
        base = self._tile(h, r0, r1)
        got = self._tile(h, r0, r1, mut)
        res = {n: t.clone() for n, t in self.want().items()}
        if keys is None:
            res["out"][r0:r1, h], res["lse"][h, r0:r1], res["dq"][r0:r1, h] = got[0], got[1], got[2]
            res["dk"][:, h // self.G] += got[3] - base[3]
            res["dv"][:, h // self.G] += got[4] - base[4]
        else:
            k0, k1 = keys
            res["dk"][k0:k1, h // self.G] += (got[3] - base[3])[k0:k1]
            res["dv"][k0:k1, h // self.G] += (got[4] - base[4])[k0:k1]
        return res

    def verdicts(self, got):
        Sq, Sk = self.out.shape[0], self.dk.shape[0]
        return NI.verdicts({n: t.numpy() for n, t in got.items()}, {n: t.numpy() for n, t in self.want().items()},
                           self.dt, Sq, Sk, self.G)


# ---------------------------------------------------------------------------------------------------------------------
# the cases and their mutants
# ---------------------------------------------------------------------------------------------------------------------
ALL5 = ("out", "lse", "dq", "dk", "dv")
FWD = ("out", "lse")
_CACHE = {}


def _case(name):
    """-> (Exact, namespace of the inputs, dict of extras).  Built once per process."""
    if name in _CACHE:
        return _CACHE[name]
    dt, D = "bfloat16", 128
    scale = D ** -0.5
    if name == "main":                                   # B1 H1 S4096 causal, C = 16: the issue's small setting
        S, C = 4096, 17
        q0 = S - QT
        rows = [q0, q0 + 1, q0 + 100, S - 2, S - 1]
        parts = dict(mask=NI.mask_edges(rows, S, S, causal=True), floor=NI.key_run_edges(S, S, True, 3, "floor", tiles=(q0, 1024)),
                     per=NI.key_run_edges(S, S, True, 3, "per", tiles=(q0, 1024)), block=NI.key_block_edges(S, S, True, every=4),
                     qrun=NI.query_run_edges(S, S, True, 3, every=4))
        edges = sum(parts.values(), [])
        nd = NI.make(S, S, 1, 1, D, dt, C, seed=1, edges=edges)
        mask = Mask(S, S, causal=True)
        extra = dict(q0=q0, **parts)
    elif name == "window":                               # both window bounds, not causal, Sq != Sk
        Sq, Sk, C, win = 1536, 2048, 7, (600, 100)
        q0 = 1024
        rows = [q0, q0 + 7, q0 + 255]
        nd = NI.make(Sq, Sk, 1, 1, D, dt, C, seed=2, edges=NI.mask_edges(rows, Sq, Sk, window=win))
        mask = Mask(Sq, Sk, window=win)
        extra = dict(q0=q0)
    elif name == "gqa":                                  # G = 4: a wrong query head inside the group
        S, C = 1024, 5
        nd = NI.make(S, S, 4, 1, D, dt, C, seed=3)
        mask = Mask(S, S, causal=True)
        extra = {}
    elif name == "packed":                               # two unequal sequences, causal inside each
        seqs = [(0, 700), (700, 1348)]
        S, C = 2048, 7
        s0, n = seqs[1]
        half = s0 + n // 2
        edges = [(s0 - 1, s0 - 1), (s0 - 1, s0)]            # the last row of sequence 1: its diagonal, and the key behind
        for r in (s0 + 260, s0 + 300, s0 + 400, s0 + 500):  # rows of sequence 2: its first key, and the key in front
            edges += [(r, s0), (r, s0 - 1)]
        for r in (half + 130, half + 200, half + 300, half + 380):   # rows behind the half boundary: the keys on it
            edges += [(r, half - 1), (r, half)]
        nd = NI.make(S, S, 1, 1, D, dt, C, seed=4, edges=edges, segments=seqs)
        mask = Mask(S, S, causal=True, seqs=seqs)
        extra = dict(seqs=seqs, half=half)
    ex = Exact(nd.q[0], nd.k[0], nd.v[0], nd.do[0], dt, mask, scale)
    _CACHE[name] = (ex, nd, extra)
    return _CACHE[name]


def _idx(Sk, dst, src):
    """Identity key index with tile [dst, dst + 64) reading tile [src, src + 64)."""
    m = torch.arange(Sk)
    m[dst:dst + 64] = torch.arange(src, src + 64)
    return m


def _mutants():
    """(id, case, corrupted tensors, function (Exact, extras) -> mutated result)."""
    M = []
    kt = 1024                                            # the key tile [1024, 1088) of the issue
    tile = lambda ex, e, mut: ex.mutated(0, e["q0"], e["q0"] + QT, mut)
    M.append(("drop-tile", "main", ALL5, lambda ex, e: tile(ex, e, dict(mult=(kt, kt + 64, 0.0)))))
    M.append(("twice-tile", "main", ALL5, lambda ex, e: tile(ex, e, dict(mult=(kt, kt + 64, 2.0)))))
    M.append(("k-with-next-v", "main", ("out", "dq", "dk", "dv"),
              lambda ex, e: tile(ex, e, dict(vmap=_idx(4096, kt, kt + 64)))))
    M.append(("k-with-prev-v", "main", ("out", "dq", "dk", "dv"),
              lambda ex, e: tile(ex, e, dict(vmap=_idx(4096, kt, kt - 64)))))
    M.append(("stale-k-tile", "main", ALL5, lambda ex, e: tile(ex, e, dict(kmap=_idx(4096, kt, kt - 64)))))
    M.append(("causal+1", "main", ALL5, lambda ex, e: tile(ex, e, dict(vis=dict(d_right=1)))))
    M.append(("causal-1", "main", ALL5, lambda ex, e: tile(ex, e, dict(vis=dict(d_right=-1)))))
    for n_, kw in (("window-left+1", dict(d_left=1)), ("window-left-1", dict(d_left=-1)),
                   ("window-right+1", dict(d_right=1)), ("window-right-1", dict(d_right=-1))):
        M.append((n_, "window", ALL5, lambda ex, e, kw=kw: tile(ex, e, dict(vis=kw))))

    def run_key(rule, which, m):                         # first / last key of a run of the last query tile's key cut
        def f(ex, e):
            key = next(j for r, j in e[rule] if r >= e["q0"] and j % 64 == (0 if which == "first" else 63))
            return tile(ex, e, dict(mult=(key, key + 1, m)))
        return f
    for rule, name in (("floor", "k_splits"), ("per", "dq_splits")):
        for which in ("first", "last"):
            for m, mn in ((0.0, "dropped"), (2.0, "twice")):
                tensors = ALL5 if rule == "floor" else ("dq",)
                M.append((f"{name}-run-{which}-key-{mn}", "main", tensors, run_key(rule, which, m)))

    def dkdv_block_key(which, m):                        # first / last key of a 128-key dK/dV block, for one query tile
        def f(ex, e):
            mid = (e["block"][len(e["block"]) // 2][1] + 1) // 128 * 128
            r, key = next(p for p in e["block"] if p[1] == (mid if which == "first" else mid - 1))
            q0 = r // QT * QT
            return ex.mutated(0, q0, q0 + QT, dict(mult=(key, key + 1, m)))
        return f
    for which in ("first", "last"):
        for m, mn in ((0.0, "dropped"), (2.0, "twice")):
            M.append((f"dkdv-block-{which}-key-{mn}", "main", ("dk", "dv"), dkdv_block_key(which, m)))

    def dkdv_run_row(which, m):                          # first / last query row of a dkdv_splits run, one key block
        def f(ex, e):
            r, key = next(p for p in e["qrun"] if p[0] % 64 == (0 if which == "first" else 63) and p[1] >= 1024)
            k0 = key // 128 * 128
            return ex.mutated(0, r, r + 1, dict(mult=(k0, k0 + 128, m)), keys=(k0, k0 + 128))
        return f
    for which in ("first", "last"):
        for m, mn in ((0.0, "dropped"), (2.0, "twice")):
            M.append((f"dkdv_splits-run-{which}-row-{mn}", "main", ("dk", "dv"), dkdv_run_row(which, m)))
    # one dK/dV item (key block [256, 384), head 1, all the rows that see it) reads the rows of head 2 of its group
    M.append(("gqa-wrong-head-dkdv-item", "gqa", ("dk", "dv"),
              lambda ex, e: ex.mutated(1, 256, 1024, dict(head=2), keys=(256, 384))))
    # a ring / merge block (the keys [2048, 4096) as the second block of two) merged twice, or not at all, for one tile
    M.append(("merge-block-twice", "main", FWD, lambda ex, e: tile(ex, e, dict(mult=(2048, 4096, 2.0)))))
    M.append(("merge-block-lost", "main", FWD, lambda ex, e: tile(ex, e, dict(mult=(2048, 4096, 0.0)))))
    M.append(("merge-first-block-lost", "main", FWD, lambda ex, e: tile(ex, e, dict(mult=(0, 2048, 0.0)))))

    def packed(kw, r0):
        return lambda ex, e: ex.mutated(0, r0(e), r0(e) + QT, dict(vis=kw) if "dup" not in kw else kw)
    in2 = lambda e: e["seqs"][1][0] + 256                # a tile inside sequence 2, before its half boundary
    M.append(("seq-first-key-lost", "packed", ALL5, packed(dict(d_first=1), in2)))
    M.append(("seq-first-key-1", "packed", ALL5, packed(dict(d_first=-1), in2)))
    end1 = lambda e: e["seqs"][0][1] - QT                # the last tile of sequence 1
    M.append(("seq-last-key-lost", "packed", ALL5, packed(dict(d_right=-1), end1)))
    M.append(("seq-last-key+1", "packed", ALL5, packed(dict(d_right=1), end1)))
    past = lambda e: e["half"] + 128                     # a tile of sequence 2 behind its half boundary
    M.append(("half-boundary-1", "packed", ALL5, packed(dict(d_half=-1), past)))
    M.append(("half-boundary+1", "packed", ALL5, lambda ex, e: ex.mutated(0, past(e), past(e) + QT, dict(dup=e["half"]))))
    return M


MUTANTS = _mutants()


def _ratios(mid):
    _, case, tensors, fn = next(m for m in MUTANTS if m[0] == mid)
    ex, _, extra = _case(case)
    return tensors, ex.verdicts(fn(ex, extra))


@pytest.mark.parametrize("mid", [m[0] for m in MUTANTS])
def test_every_mutant_fails_on_needle_inputs(mid):
    tensors, ver = _ratios(mid)
    if "out" in tensors or "lse" in tensors:
        assert not (ver["out"][0] and ver["lse"][0]), f"{mid}: a forward mutant passes out and lse: {ver}"
    for n_ in tensors:
        ok, ratio = ver[n_]
        assert not ok, f"{mid}: {n_} passes the suite's check ({ratio:.2f} of its bound)"
        assert ratio >= MARGIN, f"{mid}: {n_} fails by {ratio:.2f}x its bound only (< {MARGIN}x)"


@pytest.mark.parametrize("name", ["main", "window", "gqa", "packed"])
def test_unmutated_attention_agrees_with_the_reference_helper(name):
    ex, nd, extra = _case(name)
    m = ex.mask
    q, k, v, do = (torch.from_numpy(x) for x in (nd.q, nd.k, nd.v, nd.do))
    scale = q.shape[-1] ** -0.5
    spans = m.seqs or [(0, None)]
    for s0, n in spans:
        sl = slice(s0, None if n is None else s0 + n)
        ro, rl = ref_fwd(q[:, sl], k[:, sl], v[:, sl], scale, m.causal, m.window)
        assert float((ro[0] - ex.out[sl]).abs().max()) <= 1e-10 and float((rl[0] - ex.lse[:, sl]).abs().max()) <= 1e-10
        o16 = ro.to(torch.bfloat16)
        rdq, rdk, rdv, _ = ref_bwd(do[:, sl], q[:, sl], k[:, sl], v[:, sl], o16, rl, scale, m.causal, m.window)
        for a_, b_ in ((rdq[0], ex.dq[sl]), (rdk[0], ex.dk[sl]), (rdv[0], ex.dv[sl])):
            assert float((a_ - b_).abs().max()) <= 1e-10 * max(1.0, float(b_.abs().max()))
    # the unmutated result passes its own check exactly, and the 16-bit rounding of it passes too
    ver = ex.verdicts(ex.want())
    assert all(ok and ratio == 0.0 for ok, ratio in ver.values()), ver


@pytest.mark.parametrize("name", ["main", "window", "gqa", "packed"])
def test_needle_conditions_of_the_cpu_cases(name):
    ex, nd, _ = _case(name)
    rows = NI.sample_rows(ex.out.shape[0], 48)
    NI.assert_needle_conditions(nd, rows, 128 ** -0.5, lambda r: ex.mask.vis(r, r + 1)[0].numpy(), name)
    want = ex.want()
    for n_ in ("out", "dq", "dk", "dv"):                 # O(1) signals: the 2 % / 5 % relative tolerances bite
        t = want[n_]
        rms = float(t.square().mean().sqrt()) if n_ in ("out", "dq") else \
            float(t[torch.from_numpy(nd.needle[:, 0])].square().mean().sqrt())
        assert rms >= (0.03 if n_ == "dq" else 0.1), (name, n_, rms)     # (dq: small, its absolute tolerance decides)


# ---------------------------------------------------------------------------------------------------------------------
# S = 32768: white noise is blind, needles are not (affected rows only)
# ---------------------------------------------------------------------------------------------------------------------
def _deep(inputs, mut):
    """The last 256-row tile of B1 H1 S32768 D128 causal under `mut`: verdicts of out, lse, dq over the tile's rows, and
    the largest dk / dv error (the tile's contribution to the touched key rows) -- judged against atol alone, which is
    below any atol + rtol |want|."""
    S, D, dt = 32768, 128, "bfloat16"
    q, k, v, do = inputs
    T = {n: torch.from_numpy(np.asarray(x[0], dtype=np.float64)) for n, x in (("q", q), ("k", k), ("v", v), ("do", do))}
    mask, scale, r0 = Mask(S, S, causal=True), D ** -0.5, S - QT
    out, lse = tile_fwd_bwd(T, 0, r0, S, mask, scale)
    o16 = torch.from_numpy(round_to(out.numpy().astype(np.float32), dt).astype(np.float64))
    L = torch.zeros(1, S, dtype=torch.float64)
    dl = torch.zeros(1, S, dtype=torch.float64)
    L[0, r0:], dl[0, r0:] = lse, (T["do"][r0:, 0] * o16).sum(-1)
    base = tile_fwd_bwd(T, 0, r0, S, mask, scale, None, L, dl)
    got = tile_fwd_bwd(T, 0, r0, S, mask, scale, mut, L, dl)
    ver = NI.verdicts(dict(out=got[0].numpy(), lse=got[1].numpy(), dq=got[2].numpy()),
                      dict(out=base[0].numpy(), lse=base[1].numpy(), dq=base[2].numpy()), dt, S, S, 1)
    atol = TOL[dt]["grad"][0]
    for n_, i in (("dk", 3), ("dv", 4)):
        err = float((got[i] - base[i]).abs().max())
        ver[n_] = (err <= atol, err / atol)
    return ver, float(base[0].square().mean().sqrt())


DEEP_MUTANTS = {
    "drop": dict(mult=(1024, 1088, 0.0)),
    "twice": dict(mult=(1024, 1088, 2.0)),
    "mispair": dict(vmap=_idx(32768, 1024, 1088)),
}


@pytest.mark.parametrize("mid", list(DEEP_MUTANTS))
def test_white_noise_is_blind_at_32768(mid):
    """The pinned record: on N(0,1) inputs the mutant PASSES the checks of out, dq, dk and dv, with most of the bound to
    spare (dk / dv: even against atol alone) -- measured 0.06-0.19 of the bound, seed 0 (0.46 at the worst of six seeds).
    lse sits ON its bound and proves nothing either way: the tile holds 64 / 32768 of a row's mass times its relative
    weight (the mean of 64 log-normal weights, up to ~1.5 over 256 rows), so lse moves by ~2.9e-3 nat against a bound of
    2e-3 + 1e-4 * 10.9 = 3.1e-3 -- measured 0.94-1.04 of the bound over seeds 0, 1, 2, 3, 5 (1.7 at seed 4); the mispair
    mutant does not touch lse at all.  Hence: within a factor of two of the bound, while needles give 30-50x."""
    rs = np.random.RandomState(0)
    inputs = [round_to(rs.standard_normal((1, 32768, 1, 128)).astype(np.float32), "bfloat16") for _ in range(4)]
    ver, rms = _deep(inputs, DEEP_MUTANTS[mid])
    for n_ in ("out", "dq", "dk", "dv"):
        assert ver[n_][0] and ver[n_][1] <= 0.5, (mid, n_, ver)
    assert ver["lse"][1] <= 2.0, (mid, ver)
    assert rms < 2e-2, f"the output signal of the last tile (rms {rms:.2e}) is no longer below the absolute tolerance"


@pytest.mark.parametrize("mid", list(DEEP_MUTANTS))
def test_needles_see_the_same_mutants_at_32768(mid):
    nd = NI.make(32768, 32768, 1, 1, 128, "bfloat16", 61, seed=5)
    ver, rms = _deep([nd.q, nd.k, nd.v, nd.do], DEEP_MUTANTS[mid])
    for n_ in ("out",) + (("lse",) if mid != "mispair" else ()):
        ok, ratio = ver[n_]
        assert not ok and ratio >= MARGIN, (mid, n_, ratio)
    # (the gradients of ONE tile of ordinary rows, dout at a quarter of N(0,1), stay at 0.9-3x their bounds at this depth:
    # the margin of the gradients is the one of the table above, where the defect sits on rows and keys named as edges)
    assert rms > 0.2


def test_needle_conditions_at_32768():
    nd = NI.make(32768, 32768, 1, 1, 128, "bfloat16", 61, seed=5)
    j = np.arange(32768)
    mass, top, n = NI.assert_needle_conditions(nd, NI.sample_rows(32768, 40), 128 ** -0.5, lambda r: j <= r, "S32768 C61")
    assert n >= 40


# ---------------------------------------------------------------------------------------------------------------------
# the conditions on the inputs, for every case of the GPU table (tests/test_gpu_needle.py)
# ---------------------------------------------------------------------------------------------------------------------
import test_gpu_needle as GN  # noqa: E402


@pytest.mark.parametrize("c", GN.DENSE, ids=[c.id for c in GN.DENSE])
def test_needle_conditions_of_the_gpu_dense_table(c):
    nd = GN.make_inputs(c)
    NI.assert_needle_conditions(nd, NI.sample_rows(c.Sq, 24, c.seed), c.D ** -0.5, GN.visible_fn(c), c.id, softcap=c.softcap)


@pytest.mark.parametrize("i", range(len(GN.RING)))
def test_needle_conditions_of_the_gpu_ring_cases(i):
    Sq, Sa, Hq, Hkv, _, _, dt, _, _ = GN.RING[i]
    nd = GN.ring_inputs(Sq, Sa, Hq, Hkv, dt)
    j = np.arange(Sa + Sq)
    st = NI.needle_stats(nd, NI.sample_rows(Sq, 24), 128 ** -0.5, lambda r: j <= r + Sa)
    NI.assert_needle_conditions(nd, NI.sample_rows(Sq, 24), 128 ** -0.5, lambda r: j <= r + Sa, f"ring {i}")
    # the needle mass of the late rows is split over the two blocks: neither holds more than 90 % of it on average
    late = [r for r in NI.sample_rows(Sq, 24) if r >= Sq // 2]
    share = []
    for r in late:
        s = nd.k[0, :, 0].astype(np.float64) @ nd.q[0, r, 0].astype(np.float64) * 128 ** -0.5
        p = np.exp(np.where(j <= r + Sa, s, -np.inf) - s.max())
        share.append(p[:Sa].sum() / p.sum())
    assert 0.1 <= float(np.mean(share)) <= 0.9, (i, float(np.mean(share)))
    del st


@pytest.mark.parametrize("i", range(len(GN.PACKED)))
def test_needle_conditions_of_the_gpu_packed_cases(i):
    seqs, Hq, Hkv, D, dt = GN.PACKED[i]
    T, nd = GN.packed_inputs(seqs, Hq, Hkv, D, dt)
    rows = sorted({r for s0, n in seqs for r in (s0, s0 + n // 2, s0 + n - 1)} | set(NI.sample_rows(T, 24)))
    NI.assert_needle_conditions(nd, rows, D ** -0.5, GN._packed_visible(seqs, T), f"packed {i}")


def test_needle_conditions_of_the_gpu_layer_cases():
    g = GN.GRID
    nd = GN.grid_inputs()
    j = np.arange(g["S"])
    NI.assert_needle_conditions(nd, NI.sample_rows(g["S"], 24), g["D"] ** -0.5, lambda r: j <= r, "2x4 grid")
    cu, nd = GN.varlen_inputs()
    seqs = [(int(a), int(b - a)) for a, b in zip(cu[:-1], cu[1:])]
    T = int(cu[-1])
    NI.assert_needle_conditions(nd, NI.sample_rows(T, 24), 128 ** -0.5, GN._packed_visible(seqs, T), "varlen ring")


@pytest.mark.parametrize("cid", GN.LARGE_IDS)
def test_needle_conditions_of_the_gpu_large_cases(cid):
    """A row sample of the multi-pass shapes (the inputs are those the GPU test builds: same seed, same edges)."""
    import test_gpu_large_launch as LL
    c = LL._BY_ID[cid]
    nd = GN.large_needles(c)
    NI.assert_needle_conditions(nd, NI.sample_rows(c.Sq, 16, 1), c.D ** -0.5, GN.visible_fn(c), cid)


# ---------------------------------------------------------------------------------------------------------------------
# honest 16-bit rounding on needle inputs: the model the amplitude of dout was lowered against
# ---------------------------------------------------------------------------------------------------------------------
def bwd_16bit_model(tdo, tq, tk, tv, o16, rl, scale, causal, dt, vis=None):
    """The block backward in fp64 WITH the roundings every 16-bit flash backward performs (rounding_models.bwd_16bit_model
    without the pre-scaled K, in torch: 5 x faster than the numpy one on the 2^24-score cases of this file): P is rounded to
    the 16-bit type before dV = P^T dO and dS is formed from that P, dS is rounded before dQ = dS K and dK = dS^T Q.
    `vis`: (Sq, Sk) bool, the mask in place of `causal`."""
    B, Sq, Hq, D = tq.shape
    Sk, Hkv = tk.shape[1], tk.shape[2]
    G = Hq // Hkv
    q, do = tq.double(), tdo.double()
    k, v = tk.double().repeat_interleave(G, 2), tv.double().repeat_interleave(G, 2)
    log2e = 1.4426950408889634
    s2 = torch.einsum("bthd,bshd->bhts", q, k) * (scale * log2e)
    if vis is not None:
        s2 = s2.masked_fill(~vis, float("-inf"))
    elif causal:
        i, j = torch.arange(Sq)[:, None] + Sk - Sq, torch.arange(Sk)[None, :]
        s2 = s2.masked_fill(j > i, float("-inf"))
    fin = torch.isfinite(rl)
    p = torch.where(fin[..., None], torch.exp2(s2 - torch.where(fin, rl, torch.zeros_like(rl))[..., None] * log2e),
                    torch.zeros_like(s2))
    p16 = p.to(dt).double()
    dv = torch.einsum("bhts,bthd->bshd", p16, do).reshape(B, Sk, Hkv, G, D).sum(3)
    dp = torch.einsum("bthd,bshd->bhts", do, v)
    delta = (do * o16.double()).sum(-1).transpose(1, 2)
    ds16 = (p16 * (dp - delta[..., None])).to(dt).double()
    dq = torch.einsum("bhts,bshd->bthd", ds16, k) * scale
    dk = (torch.einsum("bhts,bthd->bshd", ds16, q) * scale).reshape(B, Sk, Hkv, G, D).sum(3)
    return dict(dq=dq.to(dt).double(), dk=dk.to(dt).double(), dv=dv.to(dt).double())


_MODEL_CASES = [c for c in GN.DENSE if c.window is None and not c.softcap and c.B * c.Hq * c.Sq * c.Sk <= 1 << 24]


@pytest.mark.parametrize("c", _MODEL_CASES, ids=[c.id for c in _MODEL_CASES])
def test_16bit_rounding_model_keeps_a_2x_margin_on_the_gpu_cases(c):
    """At dout = N(0,1) on every row the kernels miss the stated dK / dV tolerance on needle inputs by up to 1.6x, and this
    model reproduces their worst error / bound to three digits (e.g. 64-row family 1.462 dv on
    `ragged`, 0.985 dk / 0.807 dv on `row64-causal`; the other family 0.489 / 0.480 on the same inputs): rounding, not a
    lost key.  With dout lowered on ordinary rows (needle_inputs.do_mul_for) the model stays inside HALF of every bound
    -- asserted here for every dense GPU case without window or softcap of at most 2^24 scores (the larger ones repeat
    these group sizes and depths)."""
    nd = GN.make_inputs(c)
    dt = getattr(torch, c.dt)
    tq, tk, tv, tdo = (torch.from_numpy(x).to(dt) for x in (nd.q, nd.k, nd.v, nd.do))
    scale = c.D ** -0.5
    ro, rl = ref_fwd(tq, tk, tv, scale, c.causal)
    o16 = ro.to(dt)
    rdq, rdk, rdv, _ = ref_bwd(tdo, tq, tk, tv, o16, rl, scale, c.causal)
    got = bwd_16bit_model(tdo, tq, tk, tv, o16, rl, scale, c.causal, dt)
    ver = NI.verdicts({n_: t.numpy() for n_, t in got.items()}, dict(dq=rdq.numpy(), dk=rdk.numpy(), dv=rdv.numpy()),
                      c.dt, c.Sq, c.Sk, c.Hq // c.Hkv)
    assert all(ratio <= 0.5 for _, ratio in ver.values()), (c.id, ver)


# ---------------------------------------------------------------------------------------------------------------------
# a shifted diagonal (USP_ATTN_SHIFT): the helpers, the tables of tests/test_gpu_needle.py, the mutants
# ---------------------------------------------------------------------------------------------------------------------
import hashlib  # noqa: E402

import shift_ref  # noqa: E402

SHIFT_CASES = GN.SHIFTED + GN.RING_BLOCKS


def _old_mask_edges(rows, Sq, Sk, causal=False, window=None):
    """needle_inputs.mask_edges as it was before it took a shift (the diagonal hard-coded at Sk - Sq), kept here frozen."""
    left, right = (-1, -1) if window is None else (int(window[0]), int(window[1]))
    if causal:
        right = 0
    off = Sk - Sq
    out = []
    for r in rows:
        if right >= 0:
            out += [(r, r + off + right), (r, r + off + right + 1)]
        if left >= 0:
            out += [(r, r + off - left), (r, r + off - left - 1)]
    return [(r, j) for r, j in out if 0 <= j < Sk]


# sha256 of repr((classes, edge list)) of three DENSE cases, taken from the helpers BEFORE they knew a shift: the inputs are a
# deterministic function of (shape, seed, classes, edges), so equal lists are bit-identical inputs.  (The tensors themselves
# are not hashed: a BLAS that sums in another order may round one noise element the other way.)
_PINNED_EDGES = {"row64-causal": "6b15691e8eace31e", "ksplit4-window": "e501c9e2c9dc3b76", "cuts-5-3-w32": "09acd1f110e54e9d"}


def _edge_hash(c):
    C = GN.classes_for(GN._keys_seen(c.Sq, c.Sk, c.causal, c.window), c.D)
    return hashlib.sha256(repr((C, [(int(r), int(j)) for r, j in GN.edges_for(c)])).encode()).hexdigest()[:16]


def test_unshifted_inputs_are_what_they_were():
    """`shift=0` everywhere: the edge needles and class counts of three DENSE cases hash to the values recorded before the
    helpers took a shift; for EVERY dense case the mask edges equal the frozen pre-shift formula, an explicit shift of 0 changes
    nothing, and a shift without a bound is ignored."""
    for cid, want in _PINNED_EDGES.items():
        assert _edge_hash(GN._CFG[cid]) == want, cid
    for c in GN.DENSE:
        rows = NI.sample_rows(c.Sq, 10, c.seed)
        assert NI.mask_edges(rows, c.Sq, c.Sk, c.causal, c.window) == _old_mask_edges(rows, c.Sq, c.Sk, c.causal, c.window), c.id
        assert GN.edges_for(c) == GN.edges_for(c._replace(shift=0)), c.id
        assert GN._keys_seen(c.Sq, c.Sk, c.causal, c.window) == GN._keys_seen(c.Sq, c.Sk, c.causal, c.window, 0)
        if not c.causal and c.window is None:
            assert GN.edges_for(c) == GN.edges_for(c._replace(shift=77)), c.id
            assert (GN.visible_fn(c._replace(shift=77))(5) == GN.visible_fn(c)(5)).all()
    a, b = GN.make_inputs(GN._CFG["more-rows"]), GN.make_inputs(GN._CFG["more-rows"]._replace(shift=0))
    assert all(np.array_equal(getattr(a, n), getattr(b, n)) for n in ("q", "k", "v", "do"))


@pytest.mark.parametrize("c", SHIFT_CASES, ids=[c.id for c in SHIFT_CASES])
def test_shifted_helpers_agree_with_the_shifted_reference(c):
    """needle_inputs._visible / test_gpu_needle.visible_fn / Mask against tests/shift_ref.py (the GPU tests' truth); the mask
    edges are the last visible and the first invisible key of their row; the streamed key tiles of every 256-row query tile
    are exactly the tiles that hold a visible key (another range would mark the wrong cut boundaries)."""
    want = shift_ref.visible(c.Sq, c.Sk, c.causal, c.window, c.shift or 0).numpy()
    vis = GN.visible_fn(c)
    m = Mask(c.Sq, c.Sk, c.causal, c.window, shift=c.shift)
    for r in NI.sample_rows(c.Sq, 10, c.seed):
        assert (vis(r) == want[r]).all() and (m.vis(r, r + 1)[0].numpy() == want[r]).all(), (c.id, r)
        assert all(NI._visible(r, j, c.Sq, c.Sk, c.causal, c.window, c.shift or 0) == want[r, j] for j in range(0, c.Sk, 37))
    for r, j in NI.mask_edges(NI.sample_rows(c.Sq, 10, c.seed), c.Sq, c.Sk, c.causal, c.window, c.shift or 0):
        beside = [want[r, jj] for jj in (j - 1, j + 1) if 0 <= jj < c.Sk]
        assert len(beside) < 2 or any(b != want[r, j] for b in beside), (c.id, r, j)
    for q0 in range(0, c.Sq, 256):
        t0, nt = NI.key_tiles_of_query_tile(q0, 256, c.Sq, c.Sk, c.causal, c.window, c.shift or 0)
        seen = np.flatnonzero(want[q0:q0 + 256].any(0))
        if seen.size:
            assert t0 == seen[0] // 64 and nt == seen[-1] // 64 + 1, (c.id, q0, t0, nt, seen[0], seen[-1])
        else:
            assert t0 == nt, (c.id, q0, t0, nt)


@pytest.mark.parametrize("c", SHIFT_CASES, ids=[c.id for c in SHIFT_CASES])
def test_needle_conditions_of_the_gpu_shifted_tables(c):
    nd = GN.make_inputs(c)
    NI.assert_needle_conditions(nd, NI.sample_rows(c.Sq, 24, c.seed), c.D ** -0.5, GN.visible_fn(c), c.id)
    # the edge needles of the sampled rows lie on the SHIFTED mask's edges: the row sees one key of a pair and not the other
    vis = GN.visible_fn(c)
    pairs = NI.mask_edges(NI.sample_rows(c.Sq, 10, c.seed), c.Sq, c.Sk, c.causal, c.window, c.shift or 0)
    if not c.id.endswith(("all-visible", "all-visible-d64")):
        assert any(vis(r)[j] for r, j in pairs) and not all(vis(r)[j] for r, j in pairs), c.id


def test_shifted_table_covers_what_it_is_meant_to():
    """Asserted from the table itself: a deleted row fails here, on the CPU."""
    T = GN.SHIFTED
    assert all(c.shift is not None and (c.causal or c.window is not None) for c in T)
    for c in T:                                            # the shapes: >= 3 query tiles, >= 2 dK/dV blocks, >= 8 key tiles
        cut = c.k_splits > 1 or c.splits != (0, 0)
        assert c.Sq > 512 and c.Sk >= 512 and 600 <= max(c.Sq, c.Sk) <= (2048 if cut else 1300), c.id
    fam = lambda f: [c for c in T if c.family == f]
    left = lambda c: c.window is not None and c.window[0] >= 0
    right_win = lambda c: not c.causal and c.window is not None and c.window[1] > 0
    fwd = lambda k, split: any(c.fwd is not None and k in c.fwd and ((GN._SM in c.fwd) == split) for c in T)
    # ---- kernel: every launch kind that decodes the mask
    assert fwd("fwd_row64", False) and fwd("fwd_row64", True) and fwd("fwd_wave4", False) and fwd("fwd_wave8", False)
    assert any(left(c) and c.family == "wave32" and c.k_splits <= 1 for c in T)              # the window instantiation
    assert any(left(c) and c.family == "wave32" and c.k_splits > 1 for c in T)
    for k in ("dq_row64", "dq_wave8", "dkdv_row64", "dkdv_wave8"):
        assert any(c.bwd is not None and k in c.bwd for c in T), k
    assert any(c.family is None for c in T)
    # ---- bound
    assert any(c.causal and not left(c) for c in fam("row64")) and any(right_win(c) for c in fam("row64"))
    assert any(left(c) and not c.causal and c.window[1] < 0 for c in fam("wave32"))
    assert any(left(c) and (c.causal or c.window[1] >= 0) for c in fam("wave32"))
    assert not any(left(c) for c in fam("row64"))          # (the 64-row family declines a left bound that cuts)
    # ---- shift kinds, each in both families
    for f in ("row64", "wave32"):
        S = fam(f)
        assert any(c.shift > 0 for c in S) and any(c.shift < 0 for c in S), f
        assert any(c.shift % 64 for c in S), f
        for m in (64, 128, 256):
            assert any(c.shift and c.shift % m == 0 for c in S), (f, m)
        # a negative shift that empties whole leading 256-row tiles and part of the next
        assert any(c.causal and 256 < -(c.Sk - c.Sq + c.shift) < c.Sq and (c.Sk - c.Sq + c.shift) % 256 for c in S), f
        assert any(c.causal and not left(c) and c.shift >= c.Sk for c in S), f             # every key visible
    assert any(left(c) and c.window[0] < 64 and c.shift % 2 for c in fam("wave32"))          # narrower than a tile, odd shift
    # ---- rest
    assert {c.D for c in T} == {32, 64, 128} and {c.dt for c in T} == {"bfloat16", "float16"}
    assert any(c.Sq > c.Sk for c in T) and any(c.Sq < c.Sk for c in T) and any(c.B == 2 for c in T)
    assert any(c.k_splits == 3 and c.family == "row64" and c.causal for c in T)
    assert any(c.k_splits == 4 and left(c) for c in T)
    assert any(c.splits == (3, 2) and c.family == "row64" for c in T) and any(c.splits == (5, 3) and c.family == "wave32" for c in T)
    assert {c.dkdv_heads for c in T if c.Hq // c.Hkv == 4 and c.dkdv_heads} == {1, 2, 4}
    # ---- what the ring really launches: from the planner, the values at which its decisions flip
    R = GN.RING_BLOCKS
    assert all(c.Sq == c.Sk == 640 for c in R) and len({(c.causal, c.window, c.shift) for c in R}) == len(R) >= 6
    assert {c.shift for c in R} >= {None, 640, -640, 1280}
    assert any(c.window == (641, -1) and c.shift == 1280 for c in R)       # one (row, key) pair is left of that block
    assert not any(c.window in ((639, -1), (640, -1)) and c.shift == 1280 for c in R)      # ... and none at 639 / 640


def test_needle_conditions_of_the_gpu_ring_window_cases():
    """tests/test_gpu_ring_window.py: the needle inputs of the global-window ring, every window of its table."""
    import test_gpu_ring_window as RW
    from types import SimpleNamespace
    for ud, rd, w, causal in RW.RING_NEEDLE:
        c = 320 if rd == 4 else 640
        window = {"c-1": (c - 1, 0), "c": (c, 0), "c+1": (c + 1, 0)}.get(w, w)
        S = c * rd
        nd = RW.ring_needle_inputs(S, c, window, causal)
        vis = GN.visible_fn(SimpleNamespace(Sq=S, Sk=S, causal=causal, window=window))
        NI.assert_needle_conditions(nd, NI.sample_rows(S, 24, 3), 128 ** -0.5, vis, f"ring {ud}x{rd} {window}")


def _model_ratios(c, do_mul=None):
    """Worst error / bound of the honest 16-bit rounding model over a shifted case, one KV group of one batch entry at a time."""
    nd = GN.make_inputs(c if do_mul is None else c._replace(do_mul=do_mul))
    dt = getattr(torch, c.dt)
    G, scale = c.Hq // c.Hkv, c.D ** -0.5
    vis = shift_ref.visible(c.Sq, c.Sk, c.causal, c.window, c.shift or 0)
    worst = {}
    for b in range(c.B):
        for hk in range(c.Hkv):
            hs = slice(hk * G, (hk + 1) * G)
            tq, tdo = (torch.from_numpy(x[b:b + 1, :, hs]).to(dt) for x in (nd.q, nd.do))
            tk, tv = (torch.from_numpy(x[b:b + 1, :, hk:hk + 1]).to(dt) for x in (nd.k, nd.v))
            ro, rl = shift_ref.ref_fwd(tq, tk, tv, scale, c.causal, c.window, c.shift or 0)
            o16 = ro.to(dt)
            rdq, rdk, rdv = shift_ref.ref_bwd(tdo, tq, tk, tv, o16, rl, scale, c.causal, c.window, c.shift or 0)
            got = bwd_16bit_model(tdo, tq, tk, tv, o16, rl, scale, c.causal, dt, vis=vis)
            ver = NI.verdicts({n_: t.numpy() for n_, t in got.items()}, dict(dq=rdq.numpy(), dk=rdk.numpy(), dv=rdv.numpy()),
                              c.dt, c.Sq, c.Sk, G)
            for n_, (_, ratio) in ver.items():
                worst[n_] = max(worst.get(n_, 0.0), ratio)
    return worst


@pytest.mark.parametrize("c", SHIFT_CASES, ids=[c.id for c in SHIFT_CASES])
def test_16bit_rounding_model_keeps_a_2x_margin_on_the_shifted_cases(c):
    """As for the dense table: honest rounding of P and dS stays inside HALF of every stated bound on every shifted case (where it
    did not at the default amplitude of dout, the case carries a lower `do_mul`: the tolerance is never widened)."""
    worst = _model_ratios(c)
    assert all(r <= 0.5 for r in worst.values()), (c.id, worst)


# ---- the shift mutants: one 256-row query tile of every head computes its mask from a wrong shift ----------------------------
def _shift_case(cid):
    if ("shift", cid) not in _CACHE:
        c = GN._CFG[cid]
        nd = GN.make_inputs(c)
        ex = Exact(nd.q[0], nd.k[0], nd.v[0], nd.do[0], c.dt, Mask(c.Sq, c.Sk, c.causal, c.window, shift=c.shift), c.D ** -0.5)
        _CACHE[("shift", cid)] = (c, ex)
    return _CACHE[("shift", cid)]


def _tile_all_heads(ex, r0, r1, mut):
    """Rows [r0, r1) of EVERY head under `mut` (a wrong mask decode is the same for all heads of a launch)."""
    res = {n: t.clone() for n, t in ex.want().items()}
    for h in range(ex.out.shape[1]):
        base, got = ex._tile(h, r0, r1), ex._tile(h, r0, r1, mut)
        res["out"][r0:r1, h], res["lse"][h, r0:r1], res["dq"][r0:r1, h] = got[0], got[1], got[2]
        res["dk"][:, h // ex.G] += got[3] - base[3]
        res["dv"][:, h // ex.G] += got[4] - base[4]
    return res


_A, _B2, _K4 = "sh-r64-causal+70", "sh-w4-both-100", "sh-w4-ksplit4-window"


def _shift_mutants():
    """(id, case, function cfg -> the mutation of tile_fwd_bwd).  The tile holds the sampled rows Sq // 2 - 1 and Sq // 2."""
    M = []
    for d in (1, -1):
        sg = "+1" if d > 0 else "-1"
        M.append((f"shift{sg}-right-only", _A, lambda c, d=d: dict(vis=dict(d_right=d))))
        M.append((f"shift{sg}-right-only-of-both", _B2, lambda c, d=d: dict(vis=dict(d_right=d))))
        M.append((f"shift{sg}-left-only", _B2, lambda c, d=d: dict(vis=dict(d_left=d))))
        M.append((f"shift{sg}-both", _B2, lambda c, d=d: dict(vis=dict(d_right=d, d_left=d))))
        M.append((f"shift{sg}-both-causal-window", _K4, lambda c, d=d: dict(vis=dict(d_right=d, d_left=d))))
    M.append(("shift-on-right-not-on-left", _B2, lambda c: dict(vis=dict(shift_left=0))))
    M.append(("shift-on-left-not-on-right", _B2, lambda c: dict(vis=dict(shift_right=0))))
    M.append(("shift-wrong-sign", _A, lambda c: dict(vis=dict(shift_right=-c.shift, shift_left=-c.shift))))
    M.append(("shift-wrong-sign-both", _B2, lambda c: dict(vis=dict(shift_right=-c.shift, shift_left=-c.shift))))

    def unshifted_t0(c):
        """k_splits: the first streamed tile taken from the UNSHIFTED left bound -- with a negative shift it lies behind the
        true one, and the tiles between are never streamed."""
        q0 = (c.Sq // 2) // QT * QT
        t_true, _ = NI.key_tiles_of_query_tile(q0, QT, c.Sq, c.Sk, c.causal, c.window, c.shift)
        t_wrong, _ = NI.key_tiles_of_query_tile(q0, QT, c.Sq, c.Sk, c.causal, c.window, 0)
        assert t_wrong > t_true
        return dict(mult=(t_true * 64, t_wrong * 64, 0.0))
    M.append(("k_splits-run-start-from-the-unshifted-t0", _K4, unshifted_t0))
    return M


SHIFT_MUTANTS = _shift_mutants()


@pytest.mark.parametrize("mid", [m[0] for m in SHIFT_MUTANTS])
def test_every_shift_mutant_fails_on_a_shifted_case(mid):
    _, cid, fn = next(m for m in SHIFT_MUTANTS if m[0] == mid)
    c, ex = _shift_case(cid)
    q0 = (c.Sq // 2) // QT * QT
    ver = ex.verdicts(_tile_all_heads(ex, q0, min(c.Sq, q0 + QT), fn(c)))
    for n_ in ALL5:
        ok, ratio = ver[n_]
        assert not ok, f"{mid} on {cid}: {n_} passes the suite's check ({ratio:.2f} of its bound)"
        assert ratio >= MARGIN, f"{mid} on {cid}: {n_} fails by {ratio:.2f}x its bound only (< {MARGIN}x)"


@pytest.mark.parametrize("cid", [_A, _B2, _K4])
def test_unmutated_shifted_attention_agrees_with_the_shifted_reference(cid):
    c, ex = _shift_case(cid)
    nd = GN.make_inputs(c)
    q, k, v, do = (torch.from_numpy(x[:1]) for x in (nd.q, nd.k, nd.v, nd.do))
    ro, rl = shift_ref.ref_fwd(q, k, v, c.D ** -0.5, c.causal, c.window, c.shift)
    assert float((ro[0] - ex.out).abs().max()) <= 1e-10 and float(torch.nan_to_num(rl[0] - ex.lse, nan=0.0).abs().max()) <= 1e-10
    o16 = ro.to(getattr(torch, c.dt))
    for a_, b_ in zip(shift_ref.ref_bwd(do, q, k, v, o16, rl, c.D ** -0.5, c.causal, c.window, c.shift), (ex.dq, ex.dk, ex.dv)):
        assert float((a_[0] - b_).abs().max()) <= 1e-10 * max(1.0, float(b_.abs().max()))
    ver = ex.verdicts(ex.want())
    assert all(ok and ratio == 0.0 for ok, ratio in ver.values()), ver


def table():
    """The rows of SURVEY.md section 8(c): worst error / bound per mutant and tensor."""
    lines = []
    for mid, case, tensors, _ in MUTANTS:
        _, ver = _ratios(mid)
        lines.append((mid, case, {n_: ver[n_][1] for n_ in ALL5}, tensors))
    return lines


if __name__ == "__main__":
    for mid, case, ratios, tensors in table():
        cells = " | ".join(f"{ratios[n_]:.1f}" + ("" if n_ in tensors else " (n/a)") for n_ in ALL5)
        print(f"| {mid} | {case} | {cells} |")
    rs = np.random.RandomState(0)
    wn = [round_to(rs.standard_normal((1, 32768, 1, 128)).astype(np.float32), "bfloat16") for _ in range(4)]
    nd = NI.make(32768, 32768, 1, 1, 128, "bfloat16", 61, seed=5)
    for name, inp in (("N(0,1)", wn), ("needles", [nd.q, nd.k, nd.v, nd.do])):
        for mid, mut in DEEP_MUTANTS.items():
            ver, rms = _deep(inp, mut)
            print(f"| S32768 {name} | {mid} | " + " | ".join(f"{ver[n_][1]:.2f}" for n_ in ALL5) + f" | out rms {rms:.2e} |")
