"""csrc/usp_tile_range.h -- which tiles an item of the 64-row flash kernels streams and which of them need the mask -- compiled
for the host and checked against an ENUMERATION of (row, key) pairs.  No GPU.

The mask is  row i sees key j  iff  j < Sk  and (causal launch)  j <= i + off.  For every (Sq, Sk) the test forms the matrix
j - i once, takes its minimum and maximum over every (64-row wave, 64-key tile) and (64-row tile, 128-key block / 64-key slice)
rectangle of VALID pairs -- a rectangle holds a visible pair iff its minimum is <= off, a masked one iff its maximum is > off
or it reaches past Sk -- and compares what the header answers for every off of -Sq .. Sk - 2 (usp_mask_decode.h's range), every
256-row query tile and wave, every 128-key block and slice, and every cut of 1 .. 8.  The C below only loops and calls; no
formula of the header is written out a second time, except in the large-value case, which is there to see a 32-bit wrap.
Five mutants of the header (textual substitutions) must each fail the same sweep."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "long-context-attention_amd", "csrc")
SIZES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320, 513)
TILE, BM, OWN = 64, 256, 128
CUTS = [(n, c) for n in range(1, 9) for c in range(n)]            # (cuts, cut): 36 runs
BIG = 1 << 20

SHIM = r"""
#define USP_RANGE_FN
#include "usp_tile_range.h"
enum { TILE = 64, BM = 256, OWN = 128 };
/* query side, as usp_flash_bwd_dq64.hip calls it; fwd: the forward's cuts of a query tile's keys */
void sweep_query(int Sq, int Sk, int causal, const int* offs, int n_off, int* tiles, int* runs, int* fwd) {
  const int nq = (Sq + BM - 1) / BM;
  for (int o = 0; o < n_off; ++o)
    for (int qt = 0; qt < nq; ++qt) {
      const int off = offs[o], q0 = qt * BM;
      const int nt_all = usp_tiles_holding(usp_rows_key_end(q0, BM, Sq, Sk, causal, off), TILE);
      for (int cuts = 1; cuts <= 8; ++cuts)
        for (int cut = 0; cut < cuts; ++cut) {
          const usp_tile_run r = usp_prop_cut_keys(nt_all, Sk, cuts, cut, TILE);
          *fwd++ = r.begin; *fwd++ = r.end;
        }
      for (int w = 0; w < 4; ++w) {
        const usp_query_tiles k = usp_query_tiles_of(q0, BM, q0 + 64 * w, 64, Sq, Sk, causal, off, TILE);
        *tiles++ = k.nt; *tiles++ = k.n_w; *tiles++ = k.n_full;
        for (int cuts = 1; cuts <= 8; ++cuts)
          for (int cut = 0; cut < cuts; ++cut) {
            const usp_tile_run r = usp_equal_run(0, k.nt, cuts, cut);
            *runs++ = r.begin; *runs++ = usp_clamp_to_run(k.n_full, r.begin, r.end);
            *runs++ = usp_clamp_to_run(k.n_w, r.begin, r.end); *runs++ = r.end;
          }
      }
    }
}
/* key side, as usp_flash_bwd64.hip calls it: a 128-key block, its two 64-key slices, the cuts of its query tiles */
void sweep_keys(int Sq, int Sk, int causal, const int* offs, int n_off, int* first, int* runs) {
  const int nblk = (Sk + OWN - 1) / OWN, t_end = (Sq + TILE - 1) / TILE;
  for (int o = 0; o < n_off; ++o)
    for (int blk = 0; blk < nblk; ++blk) {
      const int off = offs[o], own0 = blk * OWN;
      const int t_begin = usp_first_row_tile(own0, causal, off, t_end, TILE);
      *first++ = t_begin;
      for (int slice = 0; slice < 2; ++slice)
        for (int cuts = 1; cuts <= 8; ++cuts)
          for (int cut = 0; cut < cuts; ++cut) {
            const usp_tile_run r = usp_equal_run(t_begin, t_end, cuts, cut);
            *runs++ = r.begin; *runs++ = r.end;
            *runs++ = usp_masked_row_tiles(own0 + 64 * slice, causal, off, r.begin, r.end - r.begin, TILE);
          }
    }
}
"""


def _build(tmp, header_dir, name):
    src = tmp / f"{name}.c"
    src.write_text(SHIM)
    lib = tmp / f"lib{name}.so"
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", "-I", str(header_dir), str(src), "-o", str(lib)])
    L = ctypes.CDLL(str(lib))

    class Run(ctypes.Structure):
        _fields_ = [("begin", ctypes.c_int), ("end", ctypes.c_int)]

    class QueryTiles(ctypes.Structure):
        _fields_ = [("nt", ctypes.c_int), ("n_w", ctypes.c_int), ("n_full", ctypes.c_int)]
    L.usp_equal_run.restype = Run
    L.usp_prop_cut_keys.restype = Run
    L.usp_query_tiles_of.restype = QueryTiles
    return L


@pytest.fixture(scope="module")
def header_lib(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("tile_range"), CSRC, "range")


def _ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


@functools.lru_cache(maxsize=None)
def _enumerate(Sq, Sk):
    """min / max of j - i over the VALID pairs of every rectangle the kernels work on (computed once per shape)."""
    nq, kt, nblk, rt = -(-Sq // BM), -(-Sk // TILE), -(-Sk // OWN), -(-Sq // TILE)
    rows, keys = nq * BM, max(kt * TILE, nblk * OWN)
    d = np.arange(keys, dtype=np.int64)[None, :] - np.arange(rows, dtype=np.int64)[:, None]
    row_ok = (np.arange(rows) < Sq)[:, None]
    key_ok = (np.arange(keys) < Sk)[None, :]

    def rect(ok, rh, kw, nk):                                # -> (min, max) over [row blocks of rh][nk key blocks of kw]
        lo = np.where(ok, d, BIG)[:, :nk * kw].reshape(rows // rh, rh, nk, kw).min(axis=(1, 3))
        hi = np.where(ok, d, -BIG)[:, :nk * kw].reshape(rows // rh, rh, nk, kw).max(axis=(1, 3))
        return lo, hi
    q_lo, q_hi = rect(row_ok & key_ok, 64, TILE, kt)         # [wave][key tile]; empty rectangle: (BIG, -BIG)
    k_lo, _ = rect(row_ok & key_ok, TILE, OWN, nblk)         # [row tile][key block]
    # the slice's 64 keys as the wave holds them, whether or not they lie below Sk (the kernel masks by the causal bound alone)
    _, s_hi = rect(row_ok & np.ones_like(key_ok), TILE, 64, 2 * nblk)
    full_tile = (np.arange(kt) + 1) * TILE <= Sk
    return dict(nq=nq, kt=kt, nblk=nblk, rt=rt, q_lo=q_lo, q_hi=q_hi, k_lo=k_lo[:rt], s_hi=s_hi[:rt], full_tile=full_tile)


def _offsets(Sq, Sk, causal):
    if causal:
        return np.arange(-Sq, Sk - 1, dtype=np.int32)       # everything usp_mask_decode.h can emit
    return np.array(sorted({-Sq, Sk - Sq, Sk - 2}), dtype=np.int32)    # not read: must not matter


def _leading(flags):
    """number of leading True along the last axis"""
    return np.cumprod(flags, axis=-1).sum(axis=-1)


def _last_plus_one(flags):
    """one past the last True along the last axis, 0 if none"""
    n = flags.shape[-1]
    return np.where(flags.any(axis=-1), n - np.argmax(flags[..., ::-1], axis=-1), 0)


def check_query_side(L, Sq, Sk, causal):
    e = _enumerate(Sq, Sk)
    offs = _offsets(Sq, Sk, causal)
    n_off, nq, kt = len(offs), e["nq"], e["kt"]
    tiles = np.full((n_off, nq, 4, 3), -7, dtype=np.int32)
    runs = np.full((n_off, nq, 4, len(CUTS), 4), -7, dtype=np.int32)
    fwd = np.full((n_off, nq, len(CUTS), 2), -7, dtype=np.int32)
    L.sweep_query(Sq, Sk, int(causal), _ptr(offs), n_off, _ptr(tiles), _ptr(runs), _ptr(fwd))
    tag = (Sq, Sk, causal)
    o = offs.astype(np.int64)[:, None, None]
    some = e["q_lo"] < BIG                                   # the rectangle holds a valid pair at all
    if causal:
        any_vis = e["q_lo"][None] <= o                       # [off][wave][key tile]
        all_vis = some[None] & e["full_tile"][None, None] & (e["q_hi"][None] <= o)
    else:
        any_vis = np.broadcast_to(some[None], (n_off,) + some.shape)
        all_vis = any_vis & e["full_tile"][None, None]
    any_vis = any_vis.reshape(n_off, nq, 4, kt)
    all_vis = all_vis.reshape(n_off, nq, 4, kt)
    # nt / n_w: one past the last tile with a visible pair for a valid row of the 256-row tile / of the wave
    n_w = _last_plus_one(any_vis)
    nt = _last_plus_one(any_vis.any(axis=2))
    assert (tiles[..., 0] == nt[:, :, None]).all(), ("nt", tag)
    assert (tiles[..., 1] == n_w).all(), ("n_w", tag)
    wave_past = (np.arange(nq)[:, None] * BM + 64 * np.arange(4)[None, :]) >= Sq
    assert (tiles[..., 1][:, wave_past] == 0).all(), ("n_w of a wave past Sq", tag)
    # n_full: the leading tiles below n_w in which every pair is visible; tile n_full, when below n_w, holds a masked pair
    t = np.arange(kt)
    n_full = _leading(all_vis & (t < n_w[..., None]))
    assert (tiles[..., 2] == n_full).all(), ("n_full", tag)
    got_full = tiles[..., 2].astype(np.int64)
    idx = np.minimum(got_full, kt - 1)[..., None]
    masked_at = ~np.take_along_axis(all_vis, idx, axis=-1)[..., 0]
    assert masked_at[got_full < n_w].all(), ("tile n_full holds no masked pair", tag)
    # dq64's runs: equal runs that cover [0, nt), each cut into unmasked | masked | other waves' tiles
    tb, e_full, e_own, te = (runs[..., k].astype(np.int64) for k in range(4))
    assert (tb <= e_full).all() and (e_full <= e_own).all() and (e_own <= te).all(), ("run order", tag)
    k0 = 0
    for n in range(1, 9):
        b, en = tb[..., k0:k0 + n], te[..., k0:k0 + n]
        assert (b[..., 0] == 0).all() and (en[..., -1] == nt[:, :, None]).all() and (b[..., 1:] == en[..., :-1]).all(), ("cover", tag, n)
        k0 += n
    cls = np.where(all_vis, 0, np.where(any_vis, 1, 2))[:, :, :, None, :]                  # what the tile IS for the wave
    tt = t[None, None, None, None, :]
    said = np.where(tt < e_full[..., None], 0, np.where(tt < e_own[..., None], 1, 2))      # what the run SAYS it is
    in_run = (tt >= tb[..., None]) & (tt < te[..., None])
    assert (said == cls)[in_run].all(), ("dq64 partition", tag)
    # the forward's cuts: tile boundaries, disjoint and ascending, and together every key that some row of the tile sees
    fb, fe = fwd[..., 0].astype(np.int64), fwd[..., 1].astype(np.int64)
    assert (fb % TILE == 0).all() and (fb <= fe).all() and (fe <= Sk).all() and (fb >= 0).all(), ("fwd cut bounds", tag)
    seen_tile = any_vis.any(axis=2)                                                         # [off][qt][key tile]
    k0 = 0
    for n in range(1, 9):
        b, en = fb[..., k0:k0 + n], fe[..., k0:k0 + n]
        assert (en[..., :-1] <= b[..., 1:]).all(), ("fwd cuts overlap", tag, n)
        # a key tile with a visible pair: each of its valid keys lies in some cut (a cut holds whole tiles up to Sk)
        lo_key = (t * TILE)[None, None, None, :]
        hi_key = np.minimum(t * TILE + TILE, Sk)[None, None, None, :]
        held = ((b[..., None] <= lo_key) & (en[..., None] >= hi_key)).any(axis=2)
        assert held[seen_tile].all(), ("fwd cuts lose a visible key", tag, n)
        k0 += n


def check_key_side(L, Sq, Sk, causal):
    e = _enumerate(Sq, Sk)
    offs = _offsets(Sq, Sk, causal)
    n_off, nblk, rt = len(offs), e["nblk"], e["rt"]
    first = np.full((n_off, nblk), -7, dtype=np.int32)
    runs = np.full((n_off, nblk, 2, len(CUTS), 3), -7, dtype=np.int32)
    L.sweep_keys(Sq, Sk, int(causal), _ptr(offs), n_off, _ptr(first), _ptr(runs))
    tag = (Sq, Sk, causal)
    o = offs.astype(np.int64)[:, None, None]
    k_lo = e["k_lo"].T                                       # [key block][row tile]
    pair = (k_lo[None] <= o) if causal else np.broadcast_to((k_lo < BIG)[None], (n_off, nblk, rt))
    t = np.arange(rt)
    t_begin = first.astype(np.int64)
    assert ((t_begin >= 0) & (t_begin <= rt)).all(), ("t_begin range", tag)
    # no tile below t_begin holds a visible pair with a key of the block (tiles from t_end on hold no valid row) ...
    assert not (pair & (t[None, None, :] < t_begin[..., None])).any(), ("t_begin drops a tile", tag)
    # ... and t_begin is at most one tile early
    has = pair.any(axis=-1)
    first_pair = np.argmax(pair, axis=-1)
    assert (t_begin[has] >= first_pair[has] - 1).all(), ("t_begin early", tag)
    # the slices' masked tiles, for every cut of the block's tiles
    s_hi = e["s_hi"].T.reshape(nblk, 2, rt)                  # [key block][slice][row tile]
    masked = (s_hi[None] > offs.astype(np.int64)[:, None, None, None]) if causal else np.zeros((n_off, nblk, 2, rt), bool)
    masked = masked[:, :, :, None, :]
    tb, te, n_mask = (runs[..., k].astype(np.int64) for k in range(3))
    assert ((n_mask >= 0) & (n_mask <= te - tb)).all(), ("n_mask range", tag)
    k0 = 0
    for n in range(1, 9):                                    # the runs cover [t_begin, t_end) exactly
        b, en = tb[..., k0:k0 + n], te[..., k0:k0 + n]
        assert (b[..., 0] == t_begin[:, :, None]).all() and (en[..., -1] == rt).all() and (b[..., 1:] == en[..., :-1]).all() \
            and (b <= en).all(), ("key-side cover", tag, n)
        k0 += n
    tt = t[None, None, None, None, :]
    behind = (tt >= (tb + n_mask)[..., None]) & (tt < te[..., None])
    assert not (masked & behind).any(), ("unmasked tile holds a masked pair", tag)
    last = np.clip(tb + n_mask - 1, 0, rt - 1)[..., None]
    last_masked = np.take_along_axis(np.broadcast_to(masked, behind.shape), last, axis=-1)[..., 0]
    assert last_masked[n_mask > 0].all(), ("last masked tile holds no masked pair", tag)


def check_equal_runs(L):
    for lo in (0, 1, 5):
        for n_tiles in range(0, 41):
            for cuts in range(1, 9):
                runs = [L.usp_equal_run(lo, lo + n_tiles, cuts, c) for c in range(cuts)]
                at = lo
                for r in runs:                               # disjoint, ascending, nothing between them
                    assert r.begin == at and r.end >= r.begin, (lo, n_tiles, cuts)
                    at = r.end
                assert at == lo + n_tiles, (lo, n_tiles, cuts)


def run_sweep(L):
    check_equal_runs(L)
    for Sq in SIZES:
        for Sk in SIZES:
            for causal in (False, True):
                check_query_side(L, Sq, Sk, causal)
                check_key_side(L, Sq, Sk, causal)


def test_query_tile_side_against_enumerated_pairs(header_lib):
    """nt, n_w, n_full of every 256-row tile and wave; dq64's equal runs and their unmasked | masked | idle partition; the
    forward's proportional cuts."""
    for Sq in SIZES:
        for Sk in SIZES:
            for causal in (False, True):
                check_query_side(header_lib, Sq, Sk, causal)


def test_key_block_side_against_enumerated_pairs(header_lib):
    """dkdv64: first query tile of every 128-key block, masked leading tiles of both 64-key slices, for cuts 1 .. 8."""
    for Sq in SIZES:
        for Sk in SIZES:
            for causal in (False, True):
                check_key_side(header_lib, Sq, Sk, causal)


def test_equal_runs_are_disjoint_ascending_and_cover(header_lib):
    check_equal_runs(header_lib)


def test_large_values_do_not_wrap(header_lib):
    """Sq, Sk near 2^28 (Sq + Sk < 2^29: usp_mask_decode.h), off at both ends of its range: the header's `int` arithmetic
    against the same closed forms in Python integers."""
    L = header_lib
    Sq, Sk = (1 << 28) - 70, (1 << 28) - 190
    up = lambda n: -(-n // TILE) if n > 0 else 0
    for off in (-Sq, -Sq + 1, Sk - Sq, Sk - 2):
        for q0 in (0, 256 * 1000, (Sq - 1) // 256 * 256):
            blk_end = min(min(q0 + 256, Sq) + off, Sk)
            for w in range(4):
                qw = q0 + 64 * w
                k = L.usp_query_tiles_of(q0, 256, qw, 64, Sq, Sk, 1, off, TILE)
                n_w = up(min(min(qw + 64, Sq) + off, Sk)) if qw < Sq else 0
                n_full = min(max(qw + off + 1, 0) // TILE, Sk // TILE, n_w)
                assert (k.nt, k.n_w, k.n_full) == (up(blk_end), n_w, n_full), (off, q0, w)
            nt = up(blk_end)
            for cuts in (1, 3, 8):
                for cut in range(cuts):
                    r = L.usp_prop_cut_keys(nt, Sk, cuts, cut, TILE)
                    b = cut * nt // cuts * TILE
                    en = Sk if cut == cuts - 1 else min((cut + 1) * nt // cuts * TILE, Sk)
                    assert (r.begin, r.end) == (b, max(en, b)), (off, q0, cuts, cut)
                    r = L.usp_equal_run(0, nt, cuts, cut)
                    per = -(-nt // cuts)
                    assert (r.begin, r.end) == (min(cut * per, nt), min(min(cut * per, nt) + per, nt)), (off, q0, cuts, cut)
        t_end = -(-Sq // TILE)
        for own0 in (0, 128 * 77777, (Sk - 1) // 128 * 128):
            t_begin = min(max(own0 - off, 0) // TILE, t_end)
            assert L.usp_first_row_tile(own0, 1, off, t_end, TILE) == t_begin, (off, own0)
            for ow in (own0, own0 + 64):
                n_mask = min(max(up(ow + 63 - off) - t_begin, 0), t_end - t_begin)
                assert L.usp_masked_row_tiles(ow, 1, off, t_begin, t_end - t_begin, TILE) == n_mask, (off, ow)


MUTANTS = {
    "a + 1 dropped from a bound": ("const int lim = r0 + off + 1;", "const int lim = r0 + off;"),
    "< changed to <=": ("const int wave_end = qw < Sq ?", "const int wave_end = qw <= Sq ?"),
    "the n_w clamp removed": ("  if (r.n_full > r.n_w) r.n_full = r.n_w;\n", ""),
    "ow + 63 changed to ow + 64": ("const int lim = ow + 63 - off;", "const int lim = ow + 64 - off;"),
    "a cut's ceiling division turned into a floor": ("return (hi - lo + cuts - 1) / cuts;", "return (hi - lo) / cuts;"),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_mutant_of_the_header_fails_the_sweep(tmp_path, header_lib, name):
    old, new = MUTANTS[name]
    text = open(os.path.join(CSRC, "usp_tile_range.h")).read()
    assert text.count(old) == 1, f"the header no longer holds the text this mutant replaces: {old!r}"
    (tmp_path / "usp_tile_range.h").write_text(text.replace(old, new))
    mutant = _build(tmp_path, tmp_path, "mutant")
    with pytest.raises(AssertionError):
        run_sweep(mutant)
