/* usp_tile_range.h -- which tiles an item of the 64-row flash kernels streams, and which of them need the mask.  Plain C:
 * included by the kernels (usp_mfma64.hpp) and compiled as-is by tests/test_tile_range_cpu.py, which checks every function
 * against an enumeration of (row, key) pairs.
 *
 * The mask:   row i sees key j  iff  j <= i + causal_off (causal instantiation only)  and  j < n_keys,
 *             0 <= i < Sq,  0 <= j;  -Sq <= causal_off <= n_keys - 2 (usp_mask_decode.h).
 * A tile is `tile` consecutive keys (query side) or rows (key side), tile t = [t * tile, (t + 1) * tile).  Each function
 * as a property of that mask ("valid" row: i < Sq):
 *   usp_rows_key_end     one past the last key that some valid row of [r0, r0 + n_rows) sees (r0 < Sq; <= 0: it sees none)
 *   usp_tiles_holding    the number of leading tiles that hold a key below n -- with n = usp_rows_key_end: one past the last
 *                        tile with a visible pair for those rows, 0 if there is none
 *   usp_unmasked_tiles   leading key tiles in which EVERY row from r0 on sees every key (keys only: not yet cut down to the
 *                        tiles the rows need)
 *   usp_query_tiles_of   a 256-row query tile and one 64-row wave of it: nt = tiles the workgroup streams, n_w = tiles the wave
 *                        works on (0 for a wave that starts at or past Sq), n_full = leading tiles below n_w without a masked
 *                        pair; tile n_full, if below n_w, holds one
 *   usp_equal_run        cut `cut` of `cuts` of the tiles [lo, hi): runs of equal length (the last ones shorter or empty),
 *                        disjoint, ascending, covering [lo, hi) exactly (usp_run_length / _begin / _end: its three steps, for
 *                        a kernel whose machine code changes when it takes them as one call)
 *   usp_clamp_to_run     where a boundary of the whole range falls inside a run: with e_full = clamp(n_full), e_own =
 *                        clamp(n_w), the run [tb, te) is [tb, e_full) unmasked, [e_full, e_own) masked, [e_own, te) tiles of
 *                        other waves
 *   usp_prop_cut_keys    the forward's cut of the keys a query tile sees: proportional tile boundaries (cut c starts at tile
 *                        c * nt / cuts = usp_prop_cut_tile), the LAST cut runs to n_keys; disjoint, and together they hold
 *                        every visible key
 *   usp_first_row_tile   key side: no row tile below it holds a row that sees a key >= own0; at most one tile early (it is
 *                        exact for key own0 itself), never above t_end
 *   usp_masked_row_tiles key side: the number of leading tiles of [t_begin, t_begin + n_iter) in which some row does not see
 *                        some key of [ow, ow + 64); the tiles behind them hold no such pair
 * Every sum stays in `int` for Sq + Sk < 2^29 (usp_mask_decode.h lists them). */
#ifndef USP_TILE_RANGE_H
#define USP_TILE_RANGE_H

#ifndef USP_RANGE_FN
#define USP_RANGE_FN static inline
#endif

typedef struct usp_tile_run { int begin, end; } usp_tile_run;
typedef struct usp_query_tiles { int nt, n_w, n_full; } usp_query_tiles;

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

/* nt_all = usp_tiles_holding(usp_rows_key_end(query tile)): begin = first key of the cut, end - begin = keys in it */
USP_RANGE_FN usp_tile_run usp_prop_cut_keys(int nt_all, int n_keys, int cuts, int cut, int tile) {
  usp_tile_run r;
  int ke = (cut == cuts - 1) ? n_keys : usp_prop_cut_tile(nt_all, cuts, cut + 1) * tile;
  r.begin = usp_prop_cut_tile(nt_all, cuts, cut) * tile;
  ke = ke < n_keys ? ke : n_keys;
  r.end = ke > r.begin ? ke : r.begin;
  return r;
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

/* ow: first of the wave's 64 keys */
USP_RANGE_FN int usp_masked_row_tiles(int ow, int causal, int off, int t_begin, int n_iter, int tile) {
  int n_mask = 0;
  if (causal) {
    const int lim = ow + 63 - off;                /* tiles whose first row is below lim need the mask */
    const int tm = lim > 0 ? (lim + tile - 1) / tile : 0;
    n_mask = tm - t_begin < 0 ? 0 : (tm - t_begin > n_iter ? n_iter : tm - t_begin);
  }
  return n_mask;
}

#endif
