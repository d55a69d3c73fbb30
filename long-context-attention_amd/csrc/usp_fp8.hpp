// The tile image and the operand orders of the e4m3 forward (usp_flash_fwd_fp8.hip: q, k, v of one byte per element, head dim 128).
// K and V are read both ways -- K by rows (A operand of S^T = K Q^T: ds_read_b128), V transposed (A operand of O^T += V^T P^T:
// ds_read_b64_tr_b8) -- from ONE image:
//   tile    64 rows x 128 dims = 64 x 128 bytes = 8 KiB, row-major; a row is 8 slots of 16 bytes, two rows share a 256-byte bank row
//   swizzle logical slot s of row r sits in physical slot s ^ swz(r); swz(r) puts row bit 1 on slot bit 2, row bit 3 on slot bit 1
//           and row bit 2 on slot bit 0.  A 16-byte piece sits at position 8 (r & 1) + (s ^ swz(r)) of 16 in its bank row:
//           by rows     a 16-lane group reads ONE logical slot of 16 consecutive rows: (r & 1, swz(r)) takes all 2 x 8 values;
//           transposed  a half-wave reads logical slots 2 dj, 2 dj + 1 (32 bytes) of the 8 rows 4 hi + {0 .. 3} + {0, 8}: row bits 0, 1
//                       and 3 vary, so (r & 1, slot bits 2-1 ^ (row bit 1, row bit 3)) names eight different 32-byte pieces.
//           (The (192, 128) family's swizzle fails the second: its rows r and r + 8 differ in slot bit 0 alone.)
//   fill    LDS-DMA, 1 KiB = 8 rows per wave instruction; wave w of 4 fills rows 16 w .. 16 w + 15 in 2 pieces.  The swizzle is
//           applied on the SOURCE side: the lane landing on physical slot p of row r fetches logical slot p ^ swz(r).  Rows behind
//           the tensor's last one read as zero through the descriptor's byte count.
// The 8-bit MFMA is v_mfma_f32_32x32x64_f8f6f4 with both operands e4m3 and no scale (the scale builtin with zero scale operands:
// hipcc selects the unscaled instruction).  A lane holds 32 bytes of an operand: M (or N) index lane & 31, and 32 of the 64 k
// indices.  WHICH k indices a byte holds never matters here: a product only needs byte j of half-wave hi to mean the same k in A
// and in B, so each product below defines its own order and loads both operands by it:
//   S^T = K Q^T   byte j of half-wave hi of k-step t <-> dim 64 t + 32 (j >> 4) + 16 hi + (j & 15): two 16-byte slots per lane, of
//                 the K row from LDS and of the Q row from memory;
//   O^T += V^T P^T  byte j of half-wave hi <-> key 32 (j >> 4) + (r & 3) + 8 (r >> 2) + 4 hi, r = j & 15: the order in which the two
//                 32-key S^T accumulator blocks hold their keys (acc_m), so the packed e4m3 P^T is the B operand as it stands; V^T
//                 is read in that order by four transposing reads of 8 keys each.
// ds_read_b64_tr_b8 (probed on the device once): the 16 lanes of a group supply the 16 8-byte chunks of an [8][16] byte block (chunk
// m = row m / 2, columns 8 (m % 2) .. + 7); lane i of the group receives column i, its 8 rows in order.
#pragma once
#include "usp_common.hpp"

namespace usp {

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(2))) int i32x2;

namespace fp8 {

constexpr int kD = 128;                    // head dim = bytes per row
constexpr int kRowB = 128;
constexpr int kRows = 64;                  // keys per streamed tile
constexpr int kTileB = kRows * kRowB;      // 8 KiB
constexpr int kLdsB = 4 * kTileB;          // Kbuf[0], Kbuf[1], Vbuf[0], Vbuf[1]: 32 KiB
constexpr int kNT = kD / 64;               // k-steps of a product over the head dim
constexpr int kNDJ = kD / 32;              // 32-wide dim blocks of the transposed accumulator
// P is handed to the conversion as 2^kPShift p: the loop takes the true running maximum before it exponentiates, so p <= 1 up to
// the rounding of one fp32 FMA and one v_exp_f32 (2^8 (1 + 2^-20) at the most) -- far below e4m3's largest finite value 448, which
// the next power of two would pass.  Probabilities down to 2^-14 stay normal, the subnormal step is 2^-9 / 2^8.
constexpr int kPShift = 8;

USP_DEV int swz(int row) { return ((row & 2) << 1) | ((row >> 2) & 2) | ((row >> 2) & 1); }

USP_DEV f32x16 mfma(i32x8 a, i32x8 b, f32x16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0, 0, 0);
#else
  return c;
#endif
}
// four fp32 -> four e4m3 bytes, round to nearest even (no saturation is relied on: the callers stay below 448)
USP_DEV int pack4(float a, float b, float c, float d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_cvt_pk_fp8_f32(c, d, __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false), true);
#else
  return 0;
#endif
}
USP_DEV i32x2 lds_read_tr8(USP_LDS const char* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_ds_read_tr8_b64_v2i32((USP_LDS i32x2*)p);
#else
  return i32x2{0, 0};
#endif
}

// per-lane byte offsets (from the tile's first row in memory) of this wave's 2 pieces; row_bytes = the tensor's row pitch
USP_DEV void stage_offsets(int (&voff)[2], int wave, int lane, int row_bytes) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rr = 16 * wave + 8 * i + (lane >> 3);
    voff[i] = rr * row_bytes + (((lane & 7) ^ swz(rr)) * 16);
  }
}
// Descriptor of the tile that starts at row `row0` of a tensor of `n_rows` rows of 128 bytes (`base` = row 0, `ss` = row pitch in
// bytes): the tile offset sits in the 64-bit base, the byte count ends behind the last valid row (none left: every lane reads 0).
USP_DEV auto tile_rsrc(const char* base, int64_t ss, int row0, int n_rows) {
  int64_t rem = (int64_t)(n_rows - 1 - row0) * ss + kD;
  rem = rem < 0 ? 0 : (rem > 0xffffffffLL ? 0xffffffffLL : rem);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(base + (int64_t)row0 * ss), 0, (int)(uint32_t)rem, 0x00020000);
}
template <class R> USP_DEV void stage_tile(R rs, USP_LDS char* tile, int wave, const int (&voff)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) lds_dma16(rs, tile + (2 * wave + i) * 1024, voff[i]);
}

// Lane-constant parts of the read addresses.  The swizzle of a row depends on its bits 1-3, which a 32-row block or a 16-row step
// does not reach, and a k-step / dim block moves slot bits the lane part does not hold, so every address of a tile is ONE lane base
// with a constant XORed in, plus an immediate for the row block:
//   rows: row 32 blk + (lane & 31), slots 4 t + hi and 4 t + 2 + hi                        -> (rows ^ 64 t), (rows ^ 64 t ^ 32)
//   tr:   row 16 e8 + 4 hi + ((i >> 1) & 3) + 8 (i >> 3), slot 2 dj + g, byte 8 (i & 1)    -> (tr ^ 32 dj) + 2048 e8
// (i = lane & 15, g = (lane >> 4) & 1, hi = lane >> 5).
struct LaneBase {
  int rows, tr;
  USP_DEV explicit LaneBase(int lane) {
    const int l31 = lane & 31, hi = lane >> 5, i = lane & 15, g = (lane >> 4) & 1;
    rows = l31 * kRowB + ((hi ^ swz(l31)) * 16);
    const int r = 4 * hi + ((i >> 1) & 3) + 8 * (i >> 3);
    tr = r * kRowB + ((g ^ swz(r)) * 16) + (i & 1) * 8;
  }
  USP_DEV void keep_opaque() { asm volatile("" : "+v"(rows), "+v"(tr)); }
};
// A operand by rows: M index = tile row 32 blk + (lane & 31), bytes in the S^T order above
USP_DEV i32x8 read_rows(USP_LDS const char* tile, const LaneBase& lb, int blk, int t) {
  const u32x4 a = *(USP_LDS const u32x4*)(tile + blk * 32 * kRowB + (lb.rows ^ (64 * t)));
  const u32x4 b = *(USP_LDS const u32x4*)(tile + blk * 32 * kRowB + (lb.rows ^ (64 * t + 32)));
  return i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
}
// A operand transposed: M index = dim 32 dj + (lane & 31), bytes = the tile's 64 keys in the P^T order above
USP_DEV i32x8 read_tr(USP_LDS const char* tile, const LaneBase& lb, int dj) {
  USP_LDS const char* at = tile + (lb.tr ^ (32 * dj));
  const i32x2 v0 = lds_read_tr8(at), v1 = lds_read_tr8(at + 2048), v2 = lds_read_tr8(at + 4096), v3 = lds_read_tr8(at + 6144);
  return i32x8{v0[0], v0[1], v1[0], v1[1], v2[0], v2[1], v3[0], v3[1]};
}
// M index (row of S^T, key of S) that accumulator register r of a 32x32 block holds in half-wave hi
USP_DEV int acc_m(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

}  // namespace fp8

// The launch (usp_flash_fwd.hip hands every usp_flash_fwd_fp8 call here): the argument block is complete but for nq / n_items.
// `out_dtype` = USP_BF16 | USP_FP16; the descales are device fp32 (B, Hq) / (B, Hkv) / (B, Hkv), NULL = 1.
// USP_OK / USP_ELAUNCH / USP_EUNSUPPORTED (a row pitch of 2^25 bytes or more).
struct FwdParams;
int launch_fwd_fp8(const FwdParams& p, const float* q_descale, const float* k_descale, const float* v_descale, int out_dtype,
                   bool causal, hipStream_t st);

}  // namespace usp
