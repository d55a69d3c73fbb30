"""csrc/usp_tile_range.h -- which tiles an item of the flash kernels streams and which of them are live and need the mask --
compiled for the host and checked against an ENUMERATION of (row, key) pairs.  No GPU.

The mask is  row i sees key j  iff  j < Sk  and (causal launch)  j <= i + off.  For every (Sq, Sk) the test forms the matrix
j - i once, takes its minimum and maximum over every (64-row wave, 64-key tile) and (64-row tile, 128-key block / 64-key slice)
rectangle of VALID pairs -- a rectangle holds a visible pair iff its minimum is <= off, a masked one iff its maximum is > off
or it reaches past Sk -- and compares what the header answers for every off of -Sq .. Sk - 2 (usp_mask_decode.h's range), every
256-row query tile and wave, every 128-key block and slice, and every cut of 1 .. 8.  The C below only loops and calls; no
formula of the header is written out a second time, except in the large-value case, which is there to see a 32-bit wrap.

The two-waves-per-SIMD ("wave32") family adds the left bound  j >= i + lo  (win_on) and its geometry: 32-row waves in 256-row
and 128-row query tiles (forward; the 256-row one is the dQ block too), the 128-key dK/dV block with 32-key slices, 64-key /
64-row tiles.  The same three functions run for it, and the wave32 sweeps below take every function with the arguments of the
kernel site that calls or mirrors it (profiles/wave32_tile_range_isa.txt).  The rectangles are contiguous, so the values j - i
of one fill [min, max]: it holds a visible pair iff max(min, lo) <= min(max, off), a hidden one iff max > off or min < lo.
(off, lo) pairs: every off against a boundary set of lo -- both ends of usp_mask_decode.h's range, every multiple of LO_STEP in
it, those +- 1 -- every lo against the same kind of set of off, and no left bound at all; the non-causal instantiation takes
every lo.  The forward's cuts (each renumbered by usp_cut_problem) take the coarser CUT_STEP.  The steps are what keeps the
module inside a minute: the wave32 sweep took 128 s with multiples of 32 / 128, and 28 s with 64 / 256 once the reference was
formed per distinct bound value; every shape of SIZES stays.
Mutants of the header (textual substitutions) must each fail the same sweep."""
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
LO_STEP, CUT_STEP = 64, 256                                       # spacing of the boundary sets (see the docstring)

SHIM = r"""
#define USP_RANGE_FN
#include "usp_tile_range.h"
enum { TILE = 64, OWN = 128 };
/* query side, as usp_flash_bwd_dq64.hip calls it (BM = 256 rows, WAVE = 64) and for the 32-row waves of a 256- or 128-row tile;
   fwd: the forward's cuts of a query tile's keys */
void sweep_query(int Sq, int Sk, int causal, int BM, int WAVE, const int* offs, int n_off, int* tiles, int* runs, int* fwd) {
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
      for (int w = 0; w < BM / WAVE; ++w) {
        const usp_query_tiles k = usp_query_tiles_of(q0, BM, q0 + WAVE * w, WAVE, Sq, Sk, causal, off, TILE);
        *tiles++ = k.nt; *tiles++ = k.n_w; *tiles++ = k.n_full;
        for (int cuts = 1; cuts <= 8; ++cuts)
          for (int cut = 0; cut < cuts; ++cut) {
            const usp_tile_run r = usp_equal_run(0, k.nt, cuts, cut);
            if (!runs) continue;
            *runs++ = r.begin; *runs++ = usp_clamp_to_run(k.n_full, r.begin, r.end);
            *runs++ = usp_clamp_to_run(k.n_w, r.begin, r.end); *runs++ = r.end;
          }
      }
    }
}
/* key side, as usp_flash_bwd64.hip calls it: a 128-key block, its two 64-key slices (WK = 64; the wave32 kernel's four 32-key
   slices: WK = 32), the cuts of its query tiles */
void sweep_keys(int Sq, int Sk, int causal, int WK, const int* offs, int n_off, int* first, int* runs) {
  const int nblk = (Sk + OWN - 1) / OWN, t_end = (Sq + TILE - 1) / TILE;
  for (int o = 0; o < n_off; ++o)
    for (int blk = 0; blk < nblk; ++blk) {
      const int off = offs[o], own0 = blk * OWN;
      const int t_begin = usp_first_row_tile(own0, causal, off, t_end, TILE);
      *first++ = t_begin;
      for (int slice = 0; slice < OWN / WK; ++slice)
        for (int cuts = 1; cuts <= 8; ++cuts)
          for (int cut = 0; cut < cuts; ++cut) {
            const usp_tile_run r = usp_equal_run(t_begin, t_end, cuts, cut);
            *runs++ = r.begin; *runs++ = r.end;
            *runs++ = usp_masked_row_tiles_of(own0 + WK * slice, WK, causal, off, r.begin, r.end - r.begin, TILE);
          }
    }
}

/* ---- the wave32 family: every function with the arguments of its kernel site (offs / los / wons: n (off, lo, win_on) triples) */
/* the equal-run cut as usp_flash_bwd_dq_body.inc takes it: usp_run_length mirrored there, then the two steps */
usp_tile_run dq_run(int lo, int hi, int cuts, int cut) {
  usp_tile_run r;
  const int per = usp_run_length(lo, hi, cuts);
  r.begin = usp_run_begin(lo, hi, per, cut);
  r.end = usp_run_end(r.begin, hi, per);
  return r;
}
/* one wave of 32 rows from qw, the problem (n_keys, off, lo) and tiles [0, nt): bit t0_tile + t of live / masked set per tile */
static void wave_tiles(int qw, int Sq, int n_keys, int causal, int off, int won, int lo, int nt, int t0_tile, unsigned* live,
                       unsigned* masked) {
  int wave_end = usp_rows_key_end(qw, 32, Sq, n_keys, causal, off);
  if (qw >= Sq) wave_end = 0;
  for (int t = 0; t < nt; ++t) {
    if (usp_key_tile_live(t * TILE, TILE, qw, wave_end, won, lo)) *live |= 1u << (t0_tile + t);
    if (usp_key_tile_masked(t * TILE, TILE, qw, 32, n_keys, causal, off, won, lo)) *masked |= 1u << (t0_tile + t);
  }
}
/* query side without cuts: the forward's workgroup of BM rows (256: the dQ block too).  blk: t_end (= nt), t0 (the forward's
   t0, dQ's t_begin), rot; wave: live, masked (bit per key tile), n_full behind the rotation */
void sweep_query32(int Sq, int Sk, int causal, int BM, const int* offs, const int* los, const int* wons, int n, int* blk,
                   unsigned* wave) {
  const int nq = (Sq + BM - 1) / BM;
  for (int c = 0; c < n; ++c)
    for (int qt = 0; qt < nq; ++qt) {
      const int off = offs[c], lo = los[c], won = wons[c], q0 = qt * BM;
      const int nt = usp_tiles_holding(usp_rows_key_end(q0, BM, Sq, Sk, causal, off), TILE);
      usp_rotation rot0 = {0, 0};
      *blk++ = nt;
      *blk++ = usp_first_key_tile(q0, won, lo, nt, TILE);
      if (won) rot0 = usp_window_rotation(q0 + BM - 1, lo, nt, 0, TILE);
      *blk++ = rot0.rot;
      for (int w = 0; w < BM / 32; ++w) {
        const int qw = q0 + 32 * w;
        unsigned live = 0, masked = 0;
        int n_full = usp_unmasked_tiles(qw, Sk, causal, off, TILE);
        if (qw + 32 > Sq) n_full = 0;                  /* the kernel's policy: a ragged wave takes the masked loop */
        if (n_full > nt) n_full = nt;
        if (won) n_full = usp_window_rotation(q0 + BM - 1, lo, nt, n_full, TILE).n_full;
        wave_tiles(qw, Sq, Sk, causal, off, won, lo, nt, 0, &live, &masked);
        *wave++ = live; *wave++ = masked; *wave++ = (unsigned)n_full;
      }
    }
}
/* the forward's cuts of a query tile's keys under a left bound, each cut as the problem of its own that the kernel then runs:
   cutv: begin, end of the 36 cuts; wave, per number of cuts: live, masked, streamed key tiles in the numbering of the whole */
void sweep_fwd_cuts32(int Sq, int Sk, int causal, int BM, const int* offs, const int* los, const int* wons, int n, int* cutv,
                      unsigned* wave) {
  const int nq = (Sq + BM - 1) / BM;
  for (int c = 0; c < n; ++c)
    for (int qt = 0; qt < nq; ++qt) {
      const int off = offs[c], lo = los[c], won = wons[c], q0 = qt * BM;
      const int nt_all = usp_tiles_holding(usp_rows_key_end(q0, BM, Sq, Sk, causal, off), TILE);
      const int t0 = usp_first_key_tile(q0, won, lo, nt_all, TILE);
      for (int cuts = 1; cuts <= 8; ++cuts) {
        unsigned* out = wave + 3 * (BM / 32) * (cuts - 1);
        for (int i = 0; i < 3 * (BM / 32); ++i) out[i] = 0;
        for (int cut = 0; cut < cuts; ++cut) {
          const usp_tile_run keys = usp_prop_cut_keys_from(t0, nt_all, Sk, cuts, cut, TILE);
          const usp_cut_bounds p = usp_cut_problem(keys, off, lo);
          const int nt = usp_tiles_holding(usp_rows_key_end(q0, BM, Sq, p.n_keys, causal, p.causal_off), TILE);
          *cutv++ = keys.begin; *cutv++ = keys.end;
          for (int w = 0; w < BM / 32; ++w) {
            wave_tiles(q0 + 32 * w, Sq, p.n_keys, causal, p.causal_off, won, p.win_lo, nt, keys.begin / TILE, out + 3 * w,
                       out + 3 * w + 1);
            for (int t = 0; t < nt; ++t) out[3 * w + 2] |= 1u << (keys.begin / TILE + t);
          }
        }
      }
      wave += 3 * (BM / 32) * 8;
    }
}
/* key side: the 128-key block's row tiles [t_begin, t_end), and per 32-key slice live / masked (bit per row tile) */
void sweep_keys32(int Sq, int Sk, int causal, const int* offs, const int* los, const int* wons, int n, int* blk, unsigned* wave) {
  const int nblk = (Sk + OWN - 1) / OWN, rt = (Sq + TILE - 1) / TILE;
  for (int c = 0; c < n; ++c)
    for (int b = 0; b < nblk; ++b) {
      const int off = offs[c], lo = los[c], won = wons[c], own0 = b * OWN;
      int t_end = rt;
      int t_begin = usp_first_row_tile(own0, causal, off, t_end, TILE);
      if (won) {
        t_end = usp_last_row_tile(own0, OWN, 1, lo, t_end, TILE);
        if (t_begin > t_end) t_begin = t_end;
      }
      *blk++ = t_begin; *blk++ = t_end;
      for (int sl = 0; sl < OWN / 32; ++sl) {
        const int ow = own0 + 32 * sl;
        unsigned live = 0, masked = 0;
        for (int t = 0; t < rt; ++t) {
          if (usp_row_tile_live(t * TILE, TILE, ow, 32, Sk, causal, off, won, lo)) live |= 1u << t;
          if (usp_row_tile_masked(t * TILE, TILE, ow, 32, causal, off, won, lo)) masked |= 1u << t;
        }
        *wave++ = live; *wave++ = masked;
      }
    }
}
"""


def _build(tmp, header_dir, name):
    src = tmp / f"{name}.c"
    src.write_text(SHIM)
    lib = tmp / f"lib{name}.so"
    subprocess.check_call(["gcc", "-O2", "-fno-semantic-interposition", "-shared", "-fPIC", "-I", str(header_dir), str(src), "-o", str(lib)])
    L = ctypes.CDLL(str(lib))

    class Run(ctypes.Structure):
        _fields_ = [("begin", ctypes.c_int), ("end", ctypes.c_int)]

    class QueryTiles(ctypes.Structure):
        _fields_ = [("nt", ctypes.c_int), ("n_w", ctypes.c_int), ("n_full", ctypes.c_int)]
    L.usp_equal_run.restype = Run
    L.dq_run.restype = Run
    L.usp_prop_cut_keys.restype = Run
    L.usp_prop_cut_keys_from.restype = Run
    L.usp_query_tiles_of.restype = QueryTiles

    class CutBounds(ctypes.Structure):
        _fields_ = [("n_keys", ctypes.c_int), ("causal_off", ctypes.c_int), ("win_lo", ctypes.c_int)]

    class Rotation(ctypes.Structure):
        _fields_ = [("rot", ctypes.c_int), ("n_full", ctypes.c_int)]
    L.usp_cut_problem.restype = CutBounds
    L.usp_cut_problem.argtypes = [Run, ctypes.c_int, ctypes.c_int]
    L.usp_window_rotation.restype = Rotation
    return L


@pytest.fixture(scope="module")
def header_lib(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("tile_range"), CSRC, "range")


def _ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


@functools.lru_cache(maxsize=None)
def _enumerate(Sq, Sk, BM=BM, WAVE=64, WK=64):
    """min / max of j - i over the VALID pairs of every rectangle the kernels work on (computed once per shape and geometry:
    WAVE-row waves of BM-row query tiles, WK-key slices of the 128-key block)."""
    nq, kt, nblk, rt = -(-Sq // BM), -(-Sk // TILE), -(-Sk // OWN), -(-Sq // TILE)
    rows, keys = nq * BM, max(kt * TILE, nblk * OWN)
    d = np.arange(keys, dtype=np.int64)[None, :] - np.arange(rows, dtype=np.int64)[:, None]
    row_ok = (np.arange(rows) < Sq)[:, None]
    key_ok = (np.arange(keys) < Sk)[None, :]

    def rect(ok, rh, kw, nk):                                # -> (min, max) over [row blocks of rh][nk key blocks of kw]
        lo = np.where(ok, d, BIG)[:, :nk * kw].reshape(rows // rh, rh, nk, kw).min(axis=(1, 3))
        hi = np.where(ok, d, -BIG)[:, :nk * kw].reshape(rows // rh, rh, nk, kw).max(axis=(1, 3))
        return lo, hi
    q_lo, q_hi = rect(row_ok & key_ok, WAVE, TILE, kt)       # [wave][key tile]; empty rectangle: (BIG, -BIG)
    k_lo, _ = rect(row_ok & key_ok, TILE, OWN, nblk)         # [row tile][key block]
    # the slice's 64 keys as the wave holds them, whether or not they lie below Sk (the kernel masks by the causal bound alone)
    _, s_hi = rect(row_ok & np.ones_like(key_ok), TILE, WK, OWN // WK * nblk)
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


def check_query_side(L, Sq, Sk, causal, BM=BM, WAVE=64):
    e = _enumerate(Sq, Sk, BM, WAVE)
    offs = _offsets(Sq, Sk, causal)
    n_off, nq, kt, NW = len(offs), e["nq"], e["kt"], BM // WAVE
    tiles = np.full((n_off, nq, NW, 3), -7, dtype=np.int32)
    runs = np.full((n_off, nq, NW, len(CUTS), 4), -7, dtype=np.int32)
    fwd = np.full((n_off, nq, len(CUTS), 2), -7, dtype=np.int32)
    L.sweep_query(Sq, Sk, int(causal), BM, WAVE, _ptr(offs), n_off, _ptr(tiles), _ptr(runs) if WAVE == 64 else None, _ptr(fwd))
    tag = (Sq, Sk, causal, BM, WAVE)
    o = offs.astype(np.int64)[:, None, None]
    some = e["q_lo"] < BIG                                   # the rectangle holds a valid pair at all
    if causal:
        any_vis = e["q_lo"][None] <= o                       # [off][wave][key tile]
        all_vis = some[None] & e["full_tile"][None, None] & (e["q_hi"][None] <= o)
    else:
        any_vis = np.broadcast_to(some[None], (n_off,) + some.shape)
        all_vis = any_vis & e["full_tile"][None, None]
    any_vis = any_vis.reshape(n_off, nq, NW, kt)
    all_vis = all_vis.reshape(n_off, nq, NW, kt)
    # nt / n_w: one past the last tile with a visible pair for a valid row of the 256-row tile / of the wave
    n_w = _last_plus_one(any_vis)
    nt = _last_plus_one(any_vis.any(axis=2))
    assert (tiles[..., 0] == nt[:, :, None]).all(), ("nt", tag)
    assert (tiles[..., 1] == n_w).all(), ("n_w", tag)
    wave_past = (np.arange(nq)[:, None] * BM + WAVE * np.arange(NW)[None, :]) >= Sq
    assert (tiles[..., 1][:, wave_past] == 0).all(), ("n_w of a wave past Sq", tag)
    # n_full: the leading tiles below n_w in which every pair is visible; tile n_full, when below n_w, holds a masked pair
    t = np.arange(kt)
    n_full = _leading(all_vis & (t < n_w[..., None]))
    assert (tiles[..., 2] == n_full).all(), ("n_full", tag)
    got_full = tiles[..., 2].astype(np.int64)
    idx = np.minimum(got_full, kt - 1)[..., None]
    masked_at = ~np.take_along_axis(all_vis, idx, axis=-1)[..., 0]
    assert masked_at[got_full < n_w].all(), ("tile n_full holds no masked pair", tag)
    if WAVE == 64:
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


def check_key_side(L, Sq, Sk, causal, WK=64):
    e = _enumerate(Sq, Sk, BM, 64, WK)
    offs = _offsets(Sq, Sk, causal)
    n_off, nblk, rt, NS = len(offs), e["nblk"], e["rt"], OWN // WK
    first = np.full((n_off, nblk), -7, dtype=np.int32)
    runs = np.full((n_off, nblk, NS, len(CUTS), 3), -7, dtype=np.int32)
    L.sweep_keys(Sq, Sk, int(causal), WK, _ptr(offs), n_off, _ptr(first), _ptr(runs))
    tag = (Sq, Sk, causal, WK)
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
    s_hi = e["s_hi"].T.reshape(nblk, NS, rt)                 # [key block][slice][row tile]
    masked = (s_hi[None] > offs.astype(np.int64)[:, None, None, None]) if causal else np.zeros((n_off, nblk, NS, rt), bool)
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


# ---- the wave32 family -------------------------------------------------------------------------------------------------
def _boundary(a, b, step):
    """both ends of [a, b], every multiple of `step` in it, and those +- 1"""
    m = np.arange(-(-a // step) * step, b + 1, step)
    v = np.concatenate([[a, b], m - 1, m, m + 1])
    return np.unique(v[(v >= a) & (v <= b)])


def _combos(Sq, Sk, causal, step):
    """(off, lo, win_on) of the sweep, as int32 arrays: usp_mask_decode.h's ranges -Sq <= off <= Sk - 2, 2 - Sq <= lo <= Sk"""
    lo_all = np.arange(2 - Sq, Sk + 1)
    if not causal:                                           # off is not read
        offs, los = np.full(len(lo_all), Sk - Sq), lo_all
    else:
        off_all = np.arange(-Sq, Sk - 1)
        a = np.meshgrid(off_all, _boundary(2 - Sq, Sk, step), indexing="ij")
        b = np.meshgrid(_boundary(-Sq, Sk - 2, step), lo_all, indexing="ij")
        offs, los = (np.concatenate([x.ravel(), y.ravel()]) for x, y in zip(a, b))
    wons = np.ones(len(offs), dtype=np.int32)
    no_win = np.unique(offs)                                 # ... and every off without a left bound (lo: not read)
    offs, los, wons = np.concatenate([offs, no_win]), np.concatenate([los, np.full(len(no_win), 5)]), np.concatenate([wons, 0 * no_win])
    return offs.astype(np.int32), los.astype(np.int32), wons.astype(np.int32)


def _chunks(arrays, size=1 << 15):
    for at in range(0, len(arrays[0]), size):
        yield tuple(np.ascontiguousarray(a[at:at + size]) for a in arrays)


@functools.lru_cache(maxsize=None)
def _enumerate32(Sq, Sk):
    """min / max of j - i over the (32 rows x 64 keys) and (64 rows x 32 keys) rectangles: over their VALID pairs (empty:
    (BIG, -BIG)) and over the rectangles taken whole (rows past Sq and keys past Sk included)"""
    rows, keys = -(-Sq // 256) * 256, -(-Sk // OWN) * OWN
    d = np.arange(keys, dtype=np.int64)[None, :] - np.arange(rows, dtype=np.int64)[:, None]
    valid = (np.arange(rows) < Sq)[:, None] & (np.arange(keys) < Sk)[None, :]

    def rect(ok, rh, kw):
        shape = (rows // rh, rh, keys // kw, kw)
        return np.where(ok, d, BIG).reshape(shape).min(axis=(1, 3)), np.where(ok, d, -BIG).reshape(shape).max(axis=(1, 3))
    whole = np.ones_like(valid)
    return dict(q=rect(valid, 32, TILE), q_whole=rect(whole, 32, TILE), k=rect(valid, TILE, 32), k_whole=rect(whole, TILE, 32))


def _pack(flags):
    """bit t = flags[..., t]"""
    assert flags.shape[-1] < 31
    return (flags * (np.int32(1) << np.arange(flags.shape[-1], dtype=np.int32))).sum(axis=-1, dtype=np.int32)


def _bits_below(n):
    return (np.int32(1) << n.astype(np.int32)) - np.int32(1)


def _by_value(values, on, table, off_value):
    """table(v) -> packed flags [len(v)][...] for an array of bound values v: evaluated once per DISTINCT value, then gathered;
    off_value where the bound is not `on`"""
    uniq, inv = np.unique(values, return_inverse=True)
    return np.where(on[:, None], table(uniq.astype(np.int64)[:, None, None])[inv], off_value[None])


def _pair_truth(lo_x, hi_x, full, offs, los, wons, causal):
    """From the enumerated extremes (lo_x, hi_x)[unit][tile] of the valid pairs alone, per (off, lo, win_on) and unit, one bit per
    tile: vis = the rectangle holds a visible pair (the values j - i of a rectangle fill [min, max]: max(min, lo) <= min(max,
    off)), each = each bound on its own leaves it a pair, hid = it holds a valid pair that a bound hides, allv = it is one of
    `full` and no bound hides a pair of it"""
    some = lo_x < BIG
    right, left = np.full(len(offs), bool(causal)), wons != 0
    zero = np.zeros(lo_x.shape[0], dtype=np.int32)
    each = _by_value(offs, right, lambda o: _pack(some & (lo_x <= o)), _pack(some)) & \
        _by_value(los, left, lambda l: _pack(some & (hi_x >= l)), _pack(some))
    vis = np.where((~left | (los <= offs))[:, None], each, 0) if causal else each         # (0: no row has a window)
    hid = _by_value(offs, right, lambda o: _pack(some & (hi_x > o)), zero) | _by_value(los, left, lambda l: _pack(some & (lo_x < l)), zero)
    allv = _by_value(offs, right, lambda o: _pack(full & (hi_x <= o)), _pack(full)) & \
        _by_value(los, left, lambda l: _pack(full & (lo_x >= l)), _pack(full))
    return dict(vis=vis, each=each, hid=hid, allv=allv)


def _query32_truth(Sq, Sk, causal, offs, los, wons):
    """per (off, lo, win_on) and 32-row wave, one bit per key tile: vis, hid (a hidden pair, or the tile reaches past Sk under a
    valid row), allv (a whole tile under a wave of 32 valid rows, every pair visible); waves numbered through the 256-row tiles"""
    e = _enumerate32(Sq, Sk)
    kt, W = -(-Sk // TILE), -(-Sq // 256) * 8
    (v_lo, v_hi), (w_lo, _) = ((x[:W, :kt] for x in e[k]) for k in ("q", "q_whole"))
    full_tile = ((np.arange(kt) + 1) * TILE <= Sk)[None, :]
    wave_full = (np.arange(W) * 32 + 32 <= Sq)
    t = _pair_truth(v_lo, v_hi, (v_lo < BIG) & full_tile & wave_full[:, None], offs, los, wons, causal)
    hid = t["hid"] | _pack((np.arange(W) * 32 < Sq)[:, None] & ~full_tile)[None]
    return dict(kt=kt, vis=t["vis"], hid=hid, allv=t["allv"], wave_full=wave_full, v_hi=v_hi, w_lo=w_lo)


def check_query32(L, Sq, Sk, causal):
    """forward (query tiles of 256 and 128 rows) and dQ (256) without cuts: first key tile, rotation, live / masked per wave and
    tile"""
    for offs, los, wons in _chunks(_combos(Sq, Sk, causal, LO_STEP)):
        truth = _query32_truth(Sq, Sk, causal, offs, los, wons)
        for bm in (256, 128):
            _check_query32(L, Sq, Sk, causal, bm, offs, los, wons, truth)


def _check_query32(L, Sq, Sk, causal, bm, offs, los, wons, truth):
    nq, NW = -(-Sq // bm), bm // 32
    tag = (Sq, Sk, causal, bm)
    n, W = len(offs), nq * NW
    blk = np.full((n, nq, 3), -7, dtype=np.int32)
    wave = np.zeros((n, nq, NW, 3), dtype=np.uint32)
    L.sweep_query32(Sq, Sk, int(causal), bm, _ptr(offs), _ptr(los), _ptr(wons), n, _ptr(blk), wave.ctypes.data_as(ctypes.c_void_p))
    t = {k: (v[:, :W] if k in ("vis", "hid", "allv") else v[:W] if k != "kt" else v) for k, v in truth.items()}
    kt = t["kt"]
    live, masked, n_full = (wave[..., k].reshape(n, W).view(np.int32) for k in range(3))
    nt, t0, rot = (np.repeat(blk[..., k], NW, axis=1) for k in range(3))                        # per wave
    won, lo, off = (wons != 0)[:, None], los.astype(np.int64)[:, None], offs.astype(np.int64)[:, None]
    qw = (np.arange(W) * 32)[None, :]
    assert ((nt >= 0) & (nt <= kt) & (t0 >= 0) & (t0 <= nt)).all(), ("range", tag)
    # live: a tile with a visible pair is live (and so below nt); exact without a left bound, and with one while every
    # row of the wave has a window (lo <= off or no right bound) and the wave's first row starts below Sk
    assert not (t["vis"] & ~live).any(), ("a tile with a visible pair is not live", tag)
    exact = ~won | ((lo <= off if causal else True) & (qw + lo < Sk))
    assert (live == t["vis"])[np.broadcast_to(exact, live.shape)].all(), ("live where no pair is visible", tag)
    # masked: a streamed tile with a hidden pair is masked; exact for a wave of 32 valid rows
    assert not (t["hid"] & _bits_below(nt) & ~masked).any(), ("a tile with a hidden pair is not masked", tag)
    assert (masked == (t["hid"] & _bits_below(nt)))[:, t["wave_full"]].all(), ("masked for no pair", tag)
    # first key tile: no visible pair below it; exact for the block's first row while that row starts below Sk
    assert not (t["vis"] & _bits_below(t0)).any(), ("t0 drops a tile", tag)
    blk_hi = t["v_hi"].reshape(nq, NW, kt).max(axis=1)                                          # [query tile][key tile]
    reach = blk_hi[None] >= np.where(wons != 0, los.astype(np.int64), -BIG)[:, None, None]
    first = np.where(reach.any(axis=-1), np.argmax(reach, axis=-1), kt)
    q0 = (np.arange(nq) * bm)[None, :]
    sure = ~won | (q0 + lo < Sk)
    assert (blk[..., 1] == np.minimum(first, blk[..., 0]))[np.broadcast_to(sure, first.shape)].all(), ("t0 early", tag)
    # rotation: the walk (j + rot) % nt is a permutation; its first n_full tiles [rot, rot + n_full) are cut by no bound for
    # the wave, tile rot + n_full is (wave of 32 valid rows); tile rot - 1 is cut for the block's last row
    assert ((rot < nt) | (rot == 0)).all() and (rot + n_full <= nt).all(), ("rot range", tag)
    assert not (_bits_below(rot + n_full) & ~_bits_below(rot) & ~t["allv"]).any(), ("a main-loop tile holds a hidden pair", tag)
    more = (rot > 0) & (rot + n_full < nt) & t["wave_full"][None, :]
    assert ((t["allv"] >> (rot + n_full)) & 1 == 0)[more].all(), ("n_full behind the rotation is short", tag)
    blk_lo = t["w_lo"].reshape(nq, NW, kt).min(axis=1)
    r = blk[..., 2]
    before = np.take_along_axis(np.broadcast_to(blk_lo[None], (n, nq, kt)), np.maximum(r - 1, 0)[..., None], axis=-1)[..., 0]
    assert (before < lo)[r > 0].all(), ("rot counts a tile the left bound does not cut", tag)


def check_fwd_cuts32(L, Sq, Sk, causal):
    """the forward's cuts 1 .. 8 under a left bound: the cuts are disjoint and ascending, and each -- renumbered from its first
    key by usp_cut_problem, the wave's ranges and predicates run on (n_keys, off, lo) of the cut as the kernel runs them -- says
    of its tiles what the enumeration of the whole says of them"""
    for offs, los, wons in _chunks(_combos(Sq, Sk, causal, CUT_STEP), 1 << 13):
        truth = _query32_truth(Sq, Sk, causal, offs, los, wons)
        for bm in (256, 128):
            _check_fwd_cuts32(L, Sq, Sk, causal, bm, offs, los, wons, truth)


def _check_fwd_cuts32(L, Sq, Sk, causal, bm, offs, los, wons, truth):
    nq, NW = -(-Sq // bm), bm // 32
    tag = (Sq, Sk, causal, bm)
    n, W = len(offs), nq * NW
    cutv = np.full((n, nq, len(CUTS), 2), -7, dtype=np.int32)
    wave = np.zeros((n, nq, 8, NW, 3), dtype=np.uint32)
    L.sweep_fwd_cuts32(Sq, Sk, int(causal), bm, _ptr(offs), _ptr(los), _ptr(wons), n, _ptr(cutv), wave.ctypes.data_as(ctypes.c_void_p))
    t = {k: (v[:, :W] if k in ("vis", "hid") else v[:W]) for k, v in truth.items() if k in ("vis", "hid", "wave_full")}
    fb, fe = cutv[..., 0].astype(np.int64), cutv[..., 1].astype(np.int64)
    # (an empty cut may sit on the tile boundary behind Sk: t0 = nt_all when the left bound cuts every key)
    assert (fb % TILE == 0).all() and (fb <= fe).all() and ((fe <= Sk) | (fe == fb)).all() and (fb >= 0).all(), ("cut bounds", tag)
    k0 = 0
    for cuts in range(1, 9):
        assert (fe[..., k0:k0 + cuts - 1] <= fb[..., k0 + 1:k0 + cuts]).all(), ("cuts overlap", tag, cuts)
        k0 += cuts
    # every number of cuts at once: [combination][query tile][cuts - 1][wave]
    live, masked, streamed = (wave[..., k].view(np.int32) for k in range(3))
    vis, hid = (t[k].reshape(n, nq, 1, NW) for k in ("vis", "hid"))
    assert not (vis & ~live).any(), ("the cuts lose a visible pair", tag)
    hid_here = hid & streamed
    assert not (hid_here & ~masked).any(), ("a cut does not mask a hidden pair", tag)
    assert (masked == hid_here)[:, t["wave_full"].reshape(nq, NW)[:, None, :].repeat(8, axis=1)].all(), ("a cut masks for no pair", tag)
    assert (live == vis)[wons == 0].all(), ("a cut is live where no pair is visible", tag)


def check_keys32(L, Sq, Sk, causal):
    """dK/dV: row tiles [t_begin, t_end) of every 128-key block, live / masked of its four 32-key slices per row tile"""
    e = _enumerate32(Sq, Sk)
    nblk, rt = -(-Sk // OWN), -(-Sq // TILE)
    S = 4 * nblk
    tag = (Sq, Sk, causal)
    (v_lo, v_hi), (w_lo, w_hi) = ((x[:rt, :S].T for x in e[k]) for k in ("k", "k_whole"))            # [slice][row tile]
    has_key = (np.arange(S) * 32 < Sk)[None, :]
    for offs, los, wons in _chunks(_combos(Sq, Sk, causal, LO_STEP)):
        n = len(offs)
        blk = np.full((n, nblk, 2), -7, dtype=np.int32)
        wave = np.zeros((n, nblk, 4, 2), dtype=np.uint32)
        L.sweep_keys32(Sq, Sk, int(causal), _ptr(offs), _ptr(los), _ptr(wons), n, _ptr(blk), wave.ctypes.data_as(ctypes.c_void_p))
        valid, whole = (_pair_truth(x, y, x < BIG, offs, los, wons, causal) for x, y in ((v_lo, v_hi), (w_lo, w_hi)))
        vis, hid = valid["vis"], valid["hid"]
        live, masked = (np.ascontiguousarray(wave[..., k]).reshape(n, S).view(np.int32) for k in range(2))
        t_begin, t_end = (np.repeat(blk[..., k], 4, axis=1) for k in range(2))                       # per slice
        assert ((t_begin >= 0) & (t_begin <= t_end) & (t_end <= rt)).all(), ("range", tag)
        assert not (vis & ~(_bits_below(t_end) & ~_bits_below(t_begin))).any(), ("[t_begin, t_end) drops a tile", tag)
        assert not (vis & ~live).any(), ("a tile with a visible pair is not live", tag)
        assert not (hid & ~masked).any(), ("a tile with a hidden pair is not masked", tag)
        # both are exact for the rectangle taken whole, each bound on its own
        assert (live == np.where(has_key, whole["each"], 0)).all(), ("live, whole rectangle", tag)
        assert (masked == whole["hid"]).all(), ("masked, whole rectangle", tag)
        # t_end is exact for the block's last key, whether or not it lies below Sk
        reach = w_hi.reshape(nblk, 4, rt).max(axis=1)[None] >= np.where(wons != 0, los.astype(np.int64), -BIG)[:, None, None]
        assert (blk[..., 1] == np.minimum(_last_plus_one(reach), rt)).all(), ("t_end", tag)


def check_equal_runs(L):
    for run in (L.usp_equal_run, L.dq_run):
        for lo in (0, 1, 5):
            for n_tiles in range(0, 41):
                for cuts in range(1, 9):
                    runs = [run(lo, lo + n_tiles, cuts, c) for c in range(cuts)]
                    at = lo
                    for r in runs:                           # disjoint, ascending, nothing between them
                        assert r.begin == at and r.end >= r.begin, (lo, n_tiles, cuts)
                        at = r.end
                    assert at == lo + n_tiles, (lo, n_tiles, cuts)


def check_wave32(L, Sq, Sk, causal):
    for bm in (256, 128):                                    # NWAVES 8 and 4
        check_query_side(L, Sq, Sk, causal, bm, 32)
    check_query32(L, Sq, Sk, causal)
    check_fwd_cuts32(L, Sq, Sk, causal)
    check_key_side(L, Sq, Sk, causal, 32)
    check_keys32(L, Sq, Sk, causal)


def run_sweep(L):
    check_equal_runs(L)
    for Sq in SIZES:
        for Sk in SIZES:
            for causal in (False, True):
                check_query_side(L, Sq, Sk, causal)
                check_key_side(L, Sq, Sk, causal)
                check_wave32(L, Sq, Sk, causal)


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


def test_wave32_family_against_enumerated_pairs(header_lib):
    """32-row waves of 256- and 128-row query tiles, the 256-row dQ block, 32-key slices of the 128-key dK/dV block, under both
    bounds: ranges, the forward's cuts 1 .. 8 as problems of their own, the window kernel's rotation, live and masked tiles."""
    for Sq in SIZES:
        for Sk in SIZES:
            for causal in (False, True):
                check_wave32(header_lib, Sq, Sk, causal)


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
    # the left bound at both ends of its range: first key tile, the cut behind it and its renumbering, rotation, last row tile
    for lo in (2 - Sq, Sk - Sq - 4096, Sk):
        for q0 in (0, 256 * 1000, (Sq - 1) // 256 * 256):
            nt = up(Sk)
            t0 = min(max(q0 + lo, 0) // TILE, nt)
            assert L.usp_first_key_tile(q0, 1, lo, nt, TILE) == t0, (lo, q0)
            for cut in range(3):
                r = L.usp_prop_cut_keys_from(t0, nt, Sk, 3, cut, TILE)
                b = (t0 + cut * (nt - t0) // 3) * TILE
                en = Sk if cut == 2 else min((t0 + (cut + 1) * (nt - t0) // 3) * TILE, Sk)
                assert (r.begin, r.end) == (b, max(en, b)), (lo, q0, cut)
                c = L.usp_cut_problem(r, Sk - Sq, lo)
                assert (c.n_keys, c.causal_off, c.win_lo) == (r.end - r.begin, Sk - Sq - b, lo - b), (lo, q0, cut)
            rot = up(q0 + 255 + lo)
            w = L.usp_window_rotation(q0 + 255, lo, nt, nt, TILE)
            assert (w.rot, w.n_full) == ((0, 0) if rot >= nt else (rot, nt - rot)), (lo, q0)
        for own0 in (0, 128 * 77777, (Sk - 1) // 128 * 128):
            te = min(max((own0 + 127 - lo) // TILE + 1, 0), -(-Sq // TILE))
            assert L.usp_last_row_tile(own0, 128, 1, lo, -(-Sq // TILE), TILE) == te, (lo, own0)


MUTANTS = {
    "a + 1 dropped from a bound": ("const int lim = r0 + off + 1;", "const int lim = r0 + off;"),
    "< changed to <=": ("const int wave_end = qw < Sq ?", "const int wave_end = qw <= Sq ?"),
    "the n_w clamp removed": ("  if (r.n_full > r.n_w) r.n_full = r.n_w;\n", ""),
    "ow + 63 changed to ow + 64": ("const int lim = ow + wave_keys - 1 - off;", "const int lim = ow + wave_keys - off;"),
    "a cut's ceiling division turned into a floor": ("return (hi - lo + cuts - 1) / cuts;", "return (hi - lo) / cuts;"),
    "the wave's extent ignored": ("const int lim = ow + wave_keys - 1 - off;", "const int lim = ow + 63 - off;"),
    "first key tile: the row behind the first": ("const int first = r0 + win_lo; ", "const int first = r0 + win_lo + 1; "),
    "last row tile: a + 1 dropped": ("const int te = last >= 0 ? last / tile + 1 : 0;", "const int te = last >= 0 ? last / tile : 0;"),
    "cut under a left bound: t0 dropped from its begin": ("r.begin = (t0 + usp_prop_cut_tile(", "r.begin = (usp_prop_cut_tile("),
    "cut problem: win_lo not rebased": ("c.win_lo = win_lo - keys.begin;", "c.win_lo = win_lo;"),
    "rotation: >= changed to >": ("if (r.rot >= nt) {", "if (r.rot > nt) {"),
    "key tile live: >= changed to >": ("kt0 + tile - 1 >= qw + win_lo", "kt0 + tile - 1 > qw + win_lo"),
    "key tile masked: the wave's first row for its last": ("kt0 < qw + wave_rows - 1 + win_lo", "kt0 < qw + win_lo"),
    "row tile live: <= changed to <": ("s0 <= ow + wave_keys - 1 - win_lo", "s0 < ow + wave_keys - 1 - win_lo"),
    "row tile masked: < changed to <=": ("s0 + off < ow + wave_keys - 1)", "s0 + off <= ow + wave_keys - 1)"),
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
