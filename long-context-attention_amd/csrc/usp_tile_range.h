/* usp_tile_range.h -- which tiles an item of the flash kernels streams, and which of them are live and need the mask, for the
 * 64-row kernels and for the two-waves-per-SIMD ("wave32") family.  Plain C: included by the kernels (usp_common.hpp) and
 * compiled as-is by tests/test_tile_range_cpu.py, which checks every function against an enumeration of (row, key) pairs.
 *
 * The mask:   row i sees key j  iff  j < n_keys,  j <= i + causal_off (causal instantiation only),  j >= i + win_lo (win_on),
 *             0 <= i < Sq,  0 <= j;  -Sq <= causal_off <= n_keys - 2,  2 - Sq <= win_lo <= n_keys (usp_mask_decode.h).
 * A tile is `tile` consecutive keys (query side) or rows (key side), tile t = [t * tile, (t + 1) * tile).  Each function
 * as a property of that mask ("valid" row: i < Sq; "visible" pair: a valid row and a key it sees):
 *   usp_rows_key_end     one past the last key that some valid row of [r0, r0 + n_rows) sees under the right bound and n_keys
 *                        (r0 < Sq; <= 0: it sees none)
 *   usp_tiles_holding    the number of leading tiles that hold a key below n -- with n = usp_rows_key_end: one past the last
 *                        tile with a visible pair for those rows, 0 if there is none
 *   usp_unmasked_tiles   leading key tiles in which EVERY row from r0 on sees every key (keys only: not yet cut down to the
 *                        tiles the rows need; the left bound is not its business: usp_window_rotation)
 *   usp_query_tiles_of   a query tile and one wave of it: nt = tiles the workgroup streams, n_w = tiles the wave works on (0
 *                        for a wave that starts at or past Sq), n_full = leading tiles below n_w without a masked pair; tile
 *                        n_full, if below n_w, holds one
 *   usp_equal_run        cut `cut` of `cuts` of the tiles [lo, hi): runs of equal length (the last ones shorter or empty),
 *                        disjoint, ascending, covering [lo, hi) exactly (usp_run_length / _begin / _end: its three steps, for
 *                        a kernel whose machine code changes when it takes them as one call)
 *   usp_clamp_to_run     where a boundary of the whole range falls inside a run: with e_full = clamp(n_full), e_own =
 *                        clamp(n_w), the run [tb, te) is [tb, e_full) unmasked, [e_full, e_own) masked, [e_own, te) tiles of
 *                        other waves
 *   usp_first_key_tile   query side, left bound: no key tile below it holds a key that a row from r0 on sees; EXACT for row r0
 *                        (the row with the smallest left bound) while r0 + win_lo < n_keys; never above t_end
 *   usp_prop_cut_keys_from  the forward's cut of the keys a query tile sees, tiles [t0, nt_all) with t0 = usp_first_key_tile:
 *                        proportional tile boundaries (cut c starts at tile t0 + c * (nt_all - t0) / cuts), the LAST cut runs
 *                        to n_keys; disjoint, and together they hold every visible key (usp_prop_cut_keys: t0 = 0, no left
 *                        bound)
 *   usp_cut_problem      the cut as a problem of its own: its keys renumbered from 0, n_keys, causal_off and win_lo rebased so
 *                        that row i sees key j - begin of the cut iff it sees key j, begin <= j < end, of the whole
 *   usp_window_rotation  the window kernel walks the nt tiles in the order (j + rot) % nt: rot = leading tiles that the left
 *                        bound cuts for SOME row up to blk_last (CONSERVATIVE: rows past Sq count, rot may be one tile more
 *                        than a ragged block needs; 0 when it would reach nt: then every tile is cut); n_full = the walk
 *                        indices [0, n_full) hold tiles [rot, rot + n_full) and no bound cuts a pair of the wave in them,
 *                        given n_full_in = min(usp_unmasked_tiles of the wave, nt)
 *   usp_key_tile_live    query side, tile of keys from kt0, wave of rows from qw with wave_end = its usp_rows_key_end (0 for a
 *                        wave at or past Sq): a tile with a visible pair is live.  EXACT without a left bound; with one,
 *                        exact while win_lo <= causal_off (or no right bound) and qw + win_lo < n_keys, else CONSERVATIVE
 *                        (live, and no pair: every window of the wave is empty)
 *   usp_key_tile_masked  ... a tile of a wave with a valid row that holds a (valid row, key) pair the row does not see, or that
 *                        reaches past n_keys, is masked.  EXACT for a wave whose rows are all valid; for a ragged wave
 *                        CONSERVATIVE under the left bound (masked for the sake of a row past Sq)
 *   usp_first_row_tile   key side: no row tile below it holds a row that sees a key >= own0; at most one tile early (it is
 *                        exact for key own0 itself), never above t_end
 *   usp_last_row_tile    key side, left bound: no row tile from it on holds a row that sees a key of [own0, own0 + n_own);
 *                        EXACT for key own0 + n_own - 1, whether or not that key lies below n_keys; never above t_end
 *   usp_masked_row_tiles_of  key side: the number of leading tiles of [t_begin, t_begin + n_iter) in which some row does not see
 *                        some key of [ow, ow + wave_keys) under the right bound; the tiles behind them hold no such pair
 *                        (usp_masked_row_tiles: wave_keys = 64)
 *   usp_row_tile_live    key side, tile of rows from s0, wave of keys from ow: a tile with a visible pair is live.
 *                        CONSERVATIVE: rows past Sq and keys of the wave past n_keys count (exact for the rectangle taken
 *                        whole), and with both bounds a tile is live when each bound alone leaves it a pair
 *   usp_row_tile_masked  ... a tile that holds a (row, key of the wave) pair which a bound hides is masked.  EXACT for the
 *                        rectangle taken whole; CONSERVATIVE in that rows past Sq and keys past n_keys count (n_keys itself
 *                        needs no mask on this side: a key past it is never stored)
 * The document bound (usp_flash_fwd_doc / usp_flash_bwd_doc): a left key bound read per row instead of i + win_lo.  Two int32 arrays
 * in the launch's own coordinates, both non-decreasing and describing the same set: row_lo[i] in [0, n_keys] = the first key
 * row i sees (n_keys: none), key_hi[j] in [0, Sq] = one past the last row that sees key j under this bound (= #{i : row_lo[i]
 * <= j}).  Row i sees key j iff row_lo[i] <= j (equally: i < key_hi[j]) and the mask above without its window term holds.
 * Monotone arrays make every range two reads: the first row of a tile or wave has the smallest bound, its last valid row the
 * largest.  Values are clamped as they are read (usp_doc_clamp), so arrays that break the contract give wrong results and
 * never an index out of range.
 *   usp_doc_clamp        x cut to [0, n]
 *   usp_doc_row_lo       row_lo of row min(i, Sq - 1), clamped to [0, n_keys]   (usp_doc_key_hi: key_hi of key min(j, n_keys - 1),
 *                        clamped to [0, Sq])
 *   usp_doc_first_key_tile  query side: no key tile below it holds a key that a row from r0 on sees; EXACT for row r0; never
 *                        above t_end
 *   usp_doc_uncut_key_tile  query side: from this tile on the bound hides no key from any valid row of [r0, r0 + n_rows); EXACT
 *                        (the tile before it, if any, holds a key the last valid row does not see)
 *   usp_doc_key_tile_live   query side, wave of rows from qw with wave_end as for usp_key_tile_live, lo_first = usp_doc_row_lo
 *                        of its first row: a tile with a visible pair is live.  CONSERVATIVE: live when each bound alone
 *                        leaves the wave a pair in the tile taken whole (keys past n_keys count); EXACT inside n_keys where the key intervals of consecutive valid rows are not
 *                        empty and touch or overlap (a document mask on the diagonal block: every row sees itself)
 *   usp_doc_key_tile_masked ... the left-bound term of usp_key_tile_masked: some valid row of the wave does not see some key
 *                        of the tile, lo_last = usp_doc_row_lo of the wave's last valid row.  EXACT
 *   usp_doc_last_row_tile   key side: no row tile from it on holds a row that sees a key of [own0, own0 + n_own) under this
 *                        bound; EXACT for the last key of the block below n_keys; never above t_end
 *   usp_doc_row_tile_live   key side, wave of keys from ow, hi_last = usp_doc_key_hi of its last key below n_keys: the tile of
 *                        rows from s0 holds a row that this bound lets see a key of the wave.  EXACT for this bound alone
 *                        (the caller ANDs the causal term of usp_row_tile_live)
 *   usp_doc_row_tile_masked ... holds a (row, key of the wave) pair this bound hides, hi_first = usp_doc_key_hi of key ow.
 *                        EXACT for this bound alone; CONSERVATIVE in that rows past Sq count
 * The span bound (usp_flash_fwd_span / usp_flash_bwd_span): a right key bound read per row in place of the causal diagonal, beside
 * the document bound's left one.  Four int32 arrays in the launch's own coordinates, all non-decreasing and describing the same
 * set: row i sees key j iff row_lo[i] <= j < row_hi[i], equally key_lo[j] <= i < key_hi[j], with row_hi[i] in [0, n_keys] one
 * past the last key row i sees and key_lo[j] in [0, Sq] the first row that sees key j (= #{i : row_hi[i] <= j}).  The launch
 * runs with causal = 0: the diagonal is folded into row_hi.  A row is empty when row_lo[i] >= row_hi[i].
 *   usp_span_row_hi      row_hi of row min(i, Sq - 1), clamped to [0, n_keys]   (usp_span_key_lo: key_lo of key min(j, n_keys - 1),
 *                        clamped to [0, Sq])
 *   usp_span_key_tiles_end  query side: no key tile from it on holds a key that a valid row up to the last one sees, hi_last =
 *                        usp_span_row_hi of the last valid row; EXACT for that row; never above t_end
 *   usp_span_unmasked_key_tiles  query side: the right bound hides no key of the tiles below it from any row from the first
 *                        one on, hi_first = usp_span_row_hi of the first row.  EXACT (the tile it names, if it lies wholly below n_keys, holds a
 *                        key the first row does not see)
 *   usp_span_key_tile_live  query side, wave of rows: hi_last / lo_first = the bounds of its last valid / first row.  CONSERVATIVE:
 *                        live when each bound alone leaves the wave a pair in the tile; EXACT where the key intervals of
 *                        consecutive valid rows are not empty and touch or overlap
 *   usp_span_key_tile_masked ... the right-bound term: some valid row of the wave does not see some key of the tile, hi_first =
 *                        usp_span_row_hi of the wave's first row.  EXACT for this bound alone; CONSERVATIVE in that keys past
 *                        n_keys count (they are masked anyway)
 *   usp_span_first_row_tile key side: no row tile below it holds a row that sees a key of the block from own0 on, lo_first =
 *                        usp_span_key_lo of key own0; EXACT for that key; never above t_end
 *   usp_span_row_tile_live  key side, wave of keys, lo_first = usp_span_key_lo of its first key: the tile of rows from s0 holds a
 *                        row at or past it.  EXACT for this bound alone (the caller ANDs usp_doc_row_tile_live)
 *   usp_span_row_tile_masked ... holds a (row, key of the wave) pair this bound hides, lo_last = usp_span_key_lo of the wave's last
 *                        key below n_keys.  EXACT for this bound alone
 * Every sum stays in `int` for Sq + Sk < 2^29 (usp_mask_decode.h lists them). */
#ifndef USP_TILE_RANGE_H
#define USP_TILE_RANGE_H

#ifndef USP_RANGE_FN
#define USP_RANGE_FN static inline
#endif

typedef struct usp_tile_run { int begin, end; } usp_tile_run;
typedef struct usp_query_tiles { int nt, n_w, n_full; } usp_query_tiles;
typedef struct usp_cut_bounds { int n_keys, causal_off, win_lo; } usp_cut_bounds;
typedef struct usp_rotation { int rot, n_full; } usp_rotation;

USP_RANGE_FN int usp_rows_key_end(int r0, int n_rows, int Sq, int n_keys, int causal, int off) {
  int end = n_keys;
  if (causal) {
    const int last = (r0 + n_rows < Sq ? r0 + n_rows : Sq) - 1;
    end = last + off + 1 < n_keys ? last + off + 1 : n_keys;
  }
  return end;
}

USP_RANGE_FN int usp_tiles_holding(int n, int tile) { return n > 0 ? (n + tile - 1) / tile : 0; }

USP_RANGE_FN int usp_unmasked_tiles(int r0, int n_keys, int causal, int off, int tile) {
  int n_full = n_keys / tile;
  if (causal) {
    const int lim = r0 + off + 1;                 /* keys < lim are visible to EVERY row from r0 on */
    const int nf = lim > 0 ? lim / tile : 0;
    n_full = nf < n_full ? nf : n_full;
  }
  return n_full;
}

USP_RANGE_FN usp_query_tiles usp_query_tiles_of(int q0, int blk_rows, int qw, int wave_rows, int Sq, int n_keys, int causal,
                                                int off, int tile) {
  usp_query_tiles r;
  const int wave_end = qw < Sq ? usp_rows_key_end(qw, wave_rows, Sq, n_keys, causal, off) : 0;
  r.nt = usp_tiles_holding(usp_rows_key_end(q0, blk_rows, Sq, n_keys, causal, off), tile);
  r.n_full = usp_unmasked_tiles(qw, n_keys, causal, off, tile);
  r.n_w = usp_tiles_holding(wave_end, tile);
  if (r.n_full > r.n_w) r.n_full = r.n_w;
  return r;
}

/* the pieces of usp_equal_run: length of a run, then begin and end of run `cut` */
USP_RANGE_FN int usp_run_length(int lo, int hi, int cuts) { return (hi - lo + cuts - 1) / cuts; }
USP_RANGE_FN int usp_run_begin(int lo, int hi, int per, int cut) { return lo + cut * per < hi ? lo + cut * per : hi; }
USP_RANGE_FN int usp_run_end(int begin, int hi, int per) { return begin + per < hi ? begin + per : hi; }

USP_RANGE_FN usp_tile_run usp_equal_run(int lo, int hi, int cuts, int cut) {
  usp_tile_run r;
  const int per = usp_run_length(lo, hi, cuts);
  r.begin = usp_run_begin(lo, hi, per, cut);
  r.end = usp_run_end(r.begin, hi, per);
  return r;
}

USP_RANGE_FN int usp_clamp_to_run(int x, int tb, int te) { return x < tb ? tb : (x > te ? te : x); }

/* first tile of proportional cut `cut` of nt_all tiles (cut = cuts: one past the last) */
USP_RANGE_FN int usp_prop_cut_tile(int nt_all, int cuts, int cut) { return cut * nt_all / cuts; }

USP_RANGE_FN int usp_first_key_tile(int r0, int win_on, int win_lo, int t_end, int tile) {
  int t0 = 0;
  if (win_on) {
    const int first = r0 + win_lo;                /* the first key row r0 sees; the rows behind it start later */
    t0 = first > 0 ? first / tile : 0;
    if (t0 > t_end) t0 = t_end;
  }
  return t0;
}

/* nt_all = usp_tiles_holding(usp_rows_key_end(query tile)), t0 = usp_first_key_tile(its first row, .., nt_all, ..) (0 without
 * a left bound): begin = first key of the cut, end - begin = keys in it */
USP_RANGE_FN usp_tile_run usp_prop_cut_keys_from(int t0, int nt_all, int n_keys, int cuts, int cut, int tile) {
  usp_tile_run r;
  int ke = (cut == cuts - 1) ? n_keys : (t0 + usp_prop_cut_tile(nt_all - t0, cuts, cut + 1)) * tile;
  r.begin = (t0 + usp_prop_cut_tile(nt_all - t0, cuts, cut)) * tile;
  ke = ke < n_keys ? ke : n_keys;
  r.end = ke > r.begin ? ke : r.begin;
  return r;
}

/* without a left bound: the cut of the tiles [0, nt_all) */
USP_RANGE_FN usp_tile_run usp_prop_cut_keys(int nt_all, int n_keys, int cuts, int cut, int tile) {
  return usp_prop_cut_keys_from(0, nt_all, n_keys, cuts, cut, tile);
}

USP_RANGE_FN usp_cut_bounds usp_cut_problem(usp_tile_run keys, int causal_off, int win_lo) {
  usp_cut_bounds c;
  c.n_keys = keys.end - keys.begin;
  c.causal_off = causal_off - keys.begin;
  c.win_lo = win_lo - keys.begin;
  return c;
}

/* blk_last: the last row of the workgroup's query tile, q0 + rows - 1 */
USP_RANGE_FN usp_rotation usp_window_rotation(int blk_last, int win_lo, int nt, int n_full_in, int tile) {
  usp_rotation r;
  r.rot = usp_tiles_holding(blk_last + win_lo, tile);         /* tiles with a key below the last row's left bound */
  if (r.rot >= nt) { r.rot = 0; r.n_full = 0; }
  else r.n_full = n_full_in > r.rot ? n_full_in - r.rot : 0;
  return r;
}

USP_RANGE_FN int usp_key_tile_live(int kt0, int tile, int qw, int wave_end, int win_on, int win_lo) {
  return kt0 < wave_end && (!win_on || kt0 + tile - 1 >= qw + win_lo);
}

USP_RANGE_FN int usp_key_tile_masked(int kt0, int tile, int qw, int wave_rows, int n_keys, int causal, int off, int win_on,
                                     int win_lo) {
  return kt0 + tile > n_keys || (causal && kt0 + tile - 1 > qw + off) || (win_on && kt0 < qw + wave_rows - 1 + win_lo);
}

USP_RANGE_FN int usp_first_row_tile(int own0, int causal, int off, int t_end, int tile) {
  int t_begin = 0;
  if (causal) {
    const int first_q = own0 - off > 0 ? own0 - off : 0;      /* the first row that sees key own0 */
    t_begin = first_q / tile;
    if (t_begin > t_end) t_begin = t_end;
  }
  return t_begin;
}

USP_RANGE_FN int usp_last_row_tile(int own0, int n_own, int win_on, int win_lo, int t_end, int tile) {
  if (win_on) {
    const int last = own0 + n_own - 1 - win_lo;   /* the last row that sees the block's last key: i <= j - win_lo */
    const int te = last >= 0 ? last / tile + 1 : 0;
    t_end = te < t_end ? te : t_end;
  }
  return t_end;
}

/* ow: first of the wave's wave_keys keys */
USP_RANGE_FN int usp_masked_row_tiles_of(int ow, int wave_keys, int causal, int off, int t_begin, int n_iter, int tile) {
  int n_mask = 0;
  if (causal) {
    const int lim = ow + wave_keys - 1 - off;     /* tiles whose first row is below lim need the mask */
    const int tm = lim > 0 ? (lim + tile - 1) / tile : 0;
    n_mask = tm - t_begin < 0 ? 0 : (tm - t_begin > n_iter ? n_iter : tm - t_begin);
  }
  return n_mask;
}

/* the 64-key wave of the one-wave-per-SIMD dK/dV kernel */
USP_RANGE_FN int usp_masked_row_tiles(int ow, int causal, int off, int t_begin, int n_iter, int tile) {
  return usp_masked_row_tiles_of(ow, 64, causal, off, t_begin, n_iter, tile);
}

USP_RANGE_FN int usp_row_tile_live(int s0, int tile, int ow, int wave_keys, int n_keys, int causal, int off, int win_on,
                                   int win_lo) {
  return ow < n_keys && (!causal || s0 + tile - 1 + off >= ow) && (!win_on || s0 <= ow + wave_keys - 1 - win_lo);
}

USP_RANGE_FN int usp_row_tile_masked(int s0, int tile, int ow, int wave_keys, int causal, int off, int win_on, int win_lo) {
  return (causal && s0 + off < ow + wave_keys - 1) || (win_on && s0 + tile - 1 > ow - win_lo);
}

/* ---- the document bound: a left key bound per row (row_lo) and its transpose (key_hi), both monotone ---- */
USP_RANGE_FN int usp_doc_clamp(int x, int n) { return x < 0 ? 0 : (x > n ? n : x); }

USP_RANGE_FN int usp_doc_row_lo(const int* row_lo, int i, int Sq, int n_keys) {
  return usp_doc_clamp(row_lo[i < Sq ? i : Sq - 1], n_keys);
}

USP_RANGE_FN int usp_doc_key_hi(const int* key_hi, int j, int Sq, int n_keys) {
  return usp_doc_clamp(key_hi[j < n_keys ? j : n_keys - 1], Sq);
}

/* lo_first = usp_doc_row_lo of the item's first row */
USP_RANGE_FN int usp_doc_first_key_tile(int lo_first, int t_end, int tile) {
  const int t0 = lo_first / tile;
  return t0 < t_end ? t0 : t_end;
}

/* lo_last = usp_doc_row_lo of the last valid row of the item or wave */
USP_RANGE_FN int usp_doc_uncut_key_tile(int lo_last, int tile) { return (lo_last + tile - 1) / tile; }

USP_RANGE_FN int usp_doc_key_tile_live(int kt0, int tile, int wave_end, int lo_first) {
  return kt0 < wave_end && kt0 + tile > lo_first;
}

USP_RANGE_FN int usp_doc_key_tile_masked(int kt0, int lo_last) { return kt0 < lo_last; }

/* hi_last = usp_doc_key_hi of the block's last key below n_keys */
USP_RANGE_FN int usp_doc_last_row_tile(int hi_last, int t_end, int tile) {
  const int te = (hi_last + tile - 1) / tile;
  return te < t_end ? te : t_end;
}

USP_RANGE_FN int usp_doc_row_tile_live(int s0, int hi_last) { return s0 < hi_last; }

USP_RANGE_FN int usp_doc_row_tile_masked(int s0, int tile, int hi_first) { return s0 + tile - 1 >= hi_first; }

/* ---- the span bound: a right key bound per row (row_hi) and its transpose (key_lo), both monotone ---- */
USP_RANGE_FN int usp_span_row_hi(const int* row_hi, int i, int Sq, int n_keys) {
  return usp_doc_clamp(row_hi[i < Sq ? i : Sq - 1], n_keys);
}

USP_RANGE_FN int usp_span_key_lo(const int* key_lo, int j, int Sq, int n_keys) {
  return usp_doc_clamp(key_lo[j < n_keys ? j : n_keys - 1], Sq);
}

/* hi_last = usp_span_row_hi of the last valid row of the item */
USP_RANGE_FN int usp_span_key_tiles_end(int hi_last, int t_end, int tile) {
  const int te = hi_last > 0 ? (hi_last + tile - 1) / tile : 0;
  return te < t_end ? te : t_end;
}

/* hi_first = usp_span_row_hi of the first row of the item or wave */
USP_RANGE_FN int usp_span_unmasked_key_tiles(int hi_first, int tile) { return hi_first > 0 ? hi_first / tile : 0; }

USP_RANGE_FN int usp_span_key_tile_live(int kt0, int tile, int hi_last, int lo_first) {
  return kt0 < hi_last && kt0 + tile > lo_first;
}

USP_RANGE_FN int usp_span_key_tile_masked(int kt0, int tile, int hi_first) { return kt0 + tile > hi_first; }

/* lo_first = usp_span_key_lo of the block's first key */
USP_RANGE_FN int usp_span_first_row_tile(int lo_first, int t_end, int tile) {
  const int t0 = lo_first / tile;
  return t0 < t_end ? t0 : t_end;
}

USP_RANGE_FN int usp_span_row_tile_live(int s0, int tile, int lo_first) { return s0 + tile > lo_first; }

USP_RANGE_FN int usp_span_row_tile_masked(int s0, int lo_last) { return s0 < lo_last; }

#endif
