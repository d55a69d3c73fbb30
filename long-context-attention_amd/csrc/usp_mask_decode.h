/* usp_mask_decode.h -- the integer part of a call's mask: (Sq, Sk, causal, window, shift) -> the two numbers the flash
 * kernels decode.  Plain C: included by the host side of the library (usp_host.hpp: decode_mask) and compiled as-is by
 * tests/test_host_api.py, which sweeps it against Python integers.
 *
 * The mask of include/usp_hip.h:   row i sees key j  iff  i + diag - left <= j <= i + diag + right,
 *                                  diag = Sk - Sq + mask_shift,  0 <= i < Sq,  0 <= j < Sk,
 * `causal` sets right = 0, a negative bound is unbounded on that side, a shift without a bound moves nothing.  The kernels
 * take it as       j <= i + causal_off   (causal instantiation; causal_off = diag + right)
 *           and    j >= i + win_lo       (win_on;               win_lo = diag - left).
 * window_left / window_right may be any int (INT_MAX for "unbounded" is common) and |mask_shift| < 2^30, so both numbers are
 * formed in 64 bits here, and then
 *   - a bound that cuts no (row, key) pair of this launch is DROPPED: the non-causal instantiation (causal_off >= Sk - 1),
 *     win_on = 0 (win_lo <= 1 - Sq).  Such a call is an unbounded one to every dispatch rule, the 64-row family included;
 *   - a bound that cuts every pair is SATURATED at the first value that does: causal_off = -Sq, win_lo = Sk.
 * What a kernel receives therefore lies in  -Sq <= causal_off <= Sk - 2  and  2 - Sq <= win_lo <= Sk: far inside
 * |x| <= 2^30 + Sq + Sk, the range inside which every sum the kernels form from the two stays in `int` for Sq + Sk < 2^29
 * (rows run to Sq + 255, keys to Sk + 127, kb <= Sk + 63):
 *   forward (usp_flash_fwd_body.inc, usp_flash_fwd64.hip):  min(q0 + 256, Sq) + causal_off,  q0 + win_lo,  causal_off - kb,
 *     win_lo - kb,  blk_last + off + 1,  wav_last + off + 1,  qw + off + 1,  q0 + 255 + win_lo + 63,  qw + win_lo,
 *     qw + 31 + win_lo,  row + win_lo,  row + off;
 *   dQ (usp_flash_bwd_dq_body.inc, usp_flash_bwd_dq64.hip):  last + off + 1,  own0 + win_lo,  ow + off,  ow + 31 + win_lo,
 *     orow + win_lo,  orow + off;
 *   dK/dV (usp_flash_bwd_dkdv_body.inc, usp_flash_bwd64.hip):  own0 - off,  own0 + 127 - win_lo,  s0 + off,  ow + 31 - win_lo,
 *     ow - win_lo,  orow - win_lo - s0 - 4 hi,  orow - off;
 *   the tile ranges (usp_tile_range.h, swept on the host like this header; the bodies above call it or mirror it line for
 *     line):  last + off + 1,  r0 + off + 1,  own0 - off,  ow + wave_keys - 1 - off,  r0 + win_lo,  own0 + n_own - 1 - win_lo,
 *     causal_off - begin,  win_lo - begin (begin <= Sk + 63: an empty cut may start on the tile boundary behind Sk),
 *     blk_last + win_lo + 63,  qw + win_lo,  qw + wave_rows - 1 + win_lo,  qw + off,  s0 + 63 + off,  s0 + off,
 *     ow + wave_keys - 1 - win_lo,  ow - win_lo.
 * (Before this header the host formed Sk - Sq - window_left and += mask_shift in `int`: window_left = INT_MAX with Sq > Sk
 * or a negative shift overflowed, the dK/dV kernel's `last` wrapped negative and it streamed no row.) */
#ifndef USP_MASK_DECODE_H
#define USP_MASK_DECODE_H

#include <stdint.h>

#ifndef USP_MASK_FN
#define USP_MASK_FN static inline
#endif

typedef struct usp_mask_bounds {
  int causal;       /* the causal instantiation runs: a right bound that cuts something */
  int windowed;     /* the CALL carries a bound beyond plain causal (dense launches only), whether or not it cuts */
  int causal_off;   /* read only with `causal` */
  int win_on;       /* a left bound that cuts something */
  int win_lo;       /* read only with `win_on` */
} usp_mask_bounds;

/* has_win / has_shift: the USP_ATTN_WINDOW / USP_ATTN_SHIFT bits (the fields are read only with their bit). */
USP_MASK_FN usp_mask_bounds usp_decode_mask_bounds(int Sq, int Sk, int causal, int has_win, int window_left, int window_right,
                                                   int has_shift, int mask_shift) {
  const int wl = has_win ? window_left : -1;
  const int wr = causal ? 0 : (has_win ? window_right : -1);
  const int has_l = wl >= 0, has_r = wr >= 0;
  const int64_t diag = (int64_t)Sk - Sq + ((has_shift && (has_l || has_r)) ? mask_shift : 0);
  usp_mask_bounds m;
  m.windowed = has_l || wr > 0;
  m.causal = 0;
  m.causal_off = Sk - Sq;           /* (what an unbounded launch has always carried) */
  m.win_on = 0;
  m.win_lo = -Sq;                   /* (cuts nothing) */
  if (has_r) {
    const int64_t co = diag + wr;   /* row 0 loses key Sk - 1 first */
    if (co < (int64_t)Sk - 1) {
      m.causal = 1;
      m.causal_off = co < -(int64_t)Sq ? -Sq : (int)co;
    }
  }
  if (has_l) {
    const int64_t lo = diag - wl;   /* row Sq - 1 loses key 0 first */
    if (lo > 1 - (int64_t)Sq) {
      m.win_on = 1;
      m.win_lo = lo > (int64_t)Sk ? Sk : (int)lo;
    }
  }
  return m;
}

#endif
