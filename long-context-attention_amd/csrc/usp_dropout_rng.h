/* usp_dropout_rng.h -- the dropout mask of usp_flash_fwd_dropout / usp_flash_bwd_dropout (include/usp_hip.h): a pure function
 * of (seed, batch, QUERY head, global query row, global key), so that forward and backward, any kernel, any tiling and any
 * block of a ring regenerate the same mask.  Plain C: included by the kernels and by the host side of the library, and compiled
 * as-is (gcc) by tests/test_dropout_cpu.py, which checks it against the Random123 known answers and a Python restatement.
 *
 *   t          = min(256, max(1, lrintf((1 - p) * 256)))      keep threshold; the realised keep probability is t / 256
 *   w[4]       = Philox4x32-10(counter = (i >> 2, j >> 2, h, b), key = (seed & 0xffffffff, seed >> 32))
 *   keep(i, j) = ((w[i & 3] >> (8 * (j & 3))) & 0xff) < t
 * One call gives the 16 keep bytes of a 4-row x 4-key patch: word = row within the patch, byte = key within the patch. */
#ifndef USP_DROPOUT_RNG_H
#define USP_DROPOUT_RNG_H

#include <math.h>
#include <stdint.h>

#ifndef USP_DROPOUT_FN
#if defined(__HIPCC__)
#define USP_DROPOUT_FN __host__ __device__ static inline   /* the kernels and the host-side argument check */
#else
#define USP_DROPOUT_FN static inline
#endif
#endif

#define USP_PHILOX_M0 0xD2511F53u
#define USP_PHILOX_M1 0xCD9E8D57u
#define USP_PHILOX_W0 0x9E3779B9u
#define USP_PHILOX_W1 0xBB67AE85u

/* Keep threshold of drop probability p (0 <= p < 1): 256 keeps everything, 1 is the smallest rate served. */
USP_DROPOUT_FN int usp_dropout_threshold(float p) {
  const long t = lrintf((1.0f - p) * 256.0f);
  return (int)(t < 1 ? 1 : (t > 256 ? 256 : t));
}

/* One Philox4x32 round on c[4] with the round's key (k0, k1); (uint64_t)a * b is one v_mad_u64_u32 on the device. */
USP_DROPOUT_FN void usp_philox_round(uint32_t c[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)USP_PHILOX_M0 * c[0];
  const uint64_t p1 = (uint64_t)USP_PHILOX_M1 * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  c[0] = n0;
  c[1] = (uint32_t)p1;
  c[2] = n2;
  c[3] = (uint32_t)p0;
}

/* Philox4x32-10: ten rounds, the key bumped by the Weyl increments between them. */
USP_DROPOUT_FN void usp_philox4x32_10(const uint32_t ctr[4], uint32_t k0, uint32_t k1, uint32_t out[4]) {
  uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    usp_philox_round(c, k0, k1);
    k0 += USP_PHILOX_W0;
    k1 += USP_PHILOX_W1;
  }
  out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
}

/* The 16 keep bytes of the patch (rows 4 row_patch .. +3) x (keys 4 key_patch .. +3) of batch b, query head h. */
USP_DROPOUT_FN void usp_dropout_patch(uint64_t seed, uint32_t b, uint32_t h, uint32_t row_patch, uint32_t key_patch,
                                      uint32_t out[4]) {
  const uint32_t ctr[4] = {row_patch, key_patch, h, b};
  usp_philox4x32_10(ctr, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), out);
}

/* keep(i, j) from the patch's word i & 3: byte j & 3 below the threshold */
USP_DROPOUT_FN int usp_dropout_keep(uint32_t word, int key_in_patch, uint32_t t) {
  return ((word >> (8 * key_in_patch)) & 0xffu) < t;
}

#if defined(__cplusplus)
namespace usp {
/* What a dropout kernel receives beside its argument block (t = 0: the call has no dropout and runs the plain kernels). */
struct Dropout {
  uint32_t k0, k1;                      /* Philox key: seed & 0xffffffff, seed >> 32 */
  uint32_t row0, key0, head0;           /* global position of the launch's row 0 / key 0 / query head 0 (row0, key0 % 4 == 0) */
  uint32_t t;                           /* keep threshold, 1..255 (256 never reaches a dropout kernel); 0 = no dropout */
  float rs, irs;                        /* 256 / t and t / 256 */
};
}  /* namespace usp */
#endif

#if defined(__HIPCC__)
/* ---- device side: the keep words of one 64 x 32 score block of the two-waves-per-SIMD kernels ----------------------------
 * A lane of a 32 x 32 MFMA result holds ONE index along the lane dimension (`fixed`: its query row in the forward and dQ
 * kernels, its key in dK/dV) and, per 32-wide half h, four groups gq of four consecutive indices along the register dimension
 * (base + 32 h + 4 hi + 8 gq + (0..3)).  Group g = 4 h + gq lies in patch run_patch0 + 8 h + 2 gq of that dimension
 * (run_patch0 = base / 4 + hi), and the lane needs, of each group's patch, the four bytes where its own line crosses it.
 * The four lanes of a DPP quad hold four consecutive `fixed` indices of ONE patch (bases are multiples of 4), so they need
 * the same eight patches: lane a = lane & 3 computes groups a and 4 + a (two Philox calls, not eight) and the quad
 * exchanges words with quad_perm moves.  The result kw[g] holds the keep byte of register-dimension index m (0..3) of the
 * group in byte m: keep = usp_dropout_keep(kw[4 h + (r >> 2)], r & 3, t) for register r of half h, in all three kernels.
 *   ROWS_ON_LANE (forward, dQ): the lane's word is word (row & 3) = a of each patch, bytes = keys: taken as it is.
 *   otherwise (dK/dV): the lane needs byte (key & 3) = a of each of the four words (rows): the computing lane transposes its
 *   patch's 4 x 4 bytes first, and then the exchange is the same.
 * Every lane of the wave must be active. */
#define USP_DR_BCAST(x, g) ((uint32_t)__builtin_amdgcn_mov_dpp((int)(x), (g) * 0x55, 0xf, 0xf, false))

__device__ __forceinline__ void usp_dr_bytes_transpose(uint32_t w[4]) {
  uint32_t t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    t[k] = ((w[0] >> (8 * k)) & 0xffu) | (((w[1] >> (8 * k)) & 0xffu) << 8) | (((w[2] >> (8 * k)) & 0xffu) << 16) |
           (((w[3] >> (8 * k)) & 0xffu) << 24);
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = t[k];
}

template <bool ROWS_ON_LANE>
__device__ __forceinline__ void usp_dropout_tile_words(uint32_t k0, uint32_t k1, uint32_t b, uint32_t h, uint32_t fixed_patch,
                                                       uint32_t run_patch0, int lane, uint32_t (&kw)[8]) {
  const uint32_t a = (uint32_t)lane & 3u;
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const uint32_t run = run_patch0 + 8u * hh + 2u * a;
    uint32_t ctr[4], w[4];
    ctr[0] = ROWS_ON_LANE ? fixed_patch : run;
    ctr[1] = ROWS_ON_LANE ? run : fixed_patch;
    ctr[2] = h;
    ctr[3] = b;
    usp_philox4x32_10(ctr, k0, k1, w);
    if (!ROWS_ON_LANE) usp_dr_bytes_transpose(w);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint32_t b0, b1, b2, b3;
      if (g == 0) { b0 = USP_DR_BCAST(w[0], 0); b1 = USP_DR_BCAST(w[1], 0); b2 = USP_DR_BCAST(w[2], 0); b3 = USP_DR_BCAST(w[3], 0); }
      else if (g == 1) { b0 = USP_DR_BCAST(w[0], 1); b1 = USP_DR_BCAST(w[1], 1); b2 = USP_DR_BCAST(w[2], 1); b3 = USP_DR_BCAST(w[3], 1); }
      else if (g == 2) { b0 = USP_DR_BCAST(w[0], 2); b1 = USP_DR_BCAST(w[1], 2); b2 = USP_DR_BCAST(w[2], 2); b3 = USP_DR_BCAST(w[3], 2); }
      else { b0 = USP_DR_BCAST(w[0], 3); b1 = USP_DR_BCAST(w[1], 3); b2 = USP_DR_BCAST(w[2], 3); b3 = USP_DR_BCAST(w[3], 3); }
      kw[4 * hh + g] = a == 0 ? b0 : (a == 1 ? b1 : (a == 2 ? b2 : b3));
    }
  }
}
#endif  /* __HIPCC__ */

#endif
