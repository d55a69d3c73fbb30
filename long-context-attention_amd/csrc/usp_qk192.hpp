// The tile image of the (192, 128) head-dim kernels (usp_flash_fwd_qk192.hip, usp_flash_bwd_qk192.hip: q and k of head dim 192, v of
// head dim 128 -- multi-head latent attention).  Every streamed tensor (K, V, Q, dO) is read both ways -- by rows (A operand of a
// score product: ds_read_b128) and transposed (A operand of an accumulator product: ds_read_b64_tr_b16) -- from ONE image:
//   panel   64 rows x 64 dims = 64 x 128 bytes = 8 KiB, row-major; a row is 8 slots of 16 bytes.  A tile of K or Q is three
//           panels (dims 0-63, 64-127, 128-191: 24 KiB), a tile of V or dO two (16 KiB).  (The image of usp_d256.hpp does not carry
//           over: a 192-dim row is 24 slots, and an XOR on 5 slot bits leaves that range.)
//   swizzle logical slot s of row r sits in physical slot s ^ swz(r); swz(r) puts row bit 1 on slot bit 2, row bit 2 on slot bit 1
//           and row bit 3 on slot bit 0.  Two rows share one 256-byte bank row, so a 16-byte piece sits at position 8 (r & 1) +
//           (s ^ swz(r)) of 16 in it:
//           by rows     a 16-lane group reads ONE logical slot of 16 consecutive rows: (r & 1, swz(r)) takes all 2 x 8 values, so the
//                       group covers the 16 positions once;
//           transposed  a half-wave reads logical slots 4 x .. 4 x + 3 (64 bytes) of the 4 rows 4 m .. 4 m + 3: swz bits 0-1 only
//                       permute inside a 64-byte quarter, and (r & 1, row bit 1 = swz bit 2) names four different quarters.
//           (The plain (r >> 1) & 7 fails the second: rows 4 m and 4 m + 2 would differ in slot bit 0 alone and share a quarter.)
//   fill    LDS-DMA, 1 KiB = 8 rows of a panel per wave instruction, pieces numbered panel-major; wave w of 4 fills pieces
//           6 w .. 6 w + 5 of a three-panel tile, 4 w .. 4 w + 3 of a two-panel one.  The swizzle is applied on the SOURCE side: the
//           lane landing on physical slot p of row r fetches logical slot p ^ swz(r).  Rows behind the tensor's last one read as zero
//           through the descriptor's byte count.
// MFMA operand layouts: usp_common.hpp.
#pragma once
#include "usp_common.hpp"

namespace usp {
namespace qk192 {

constexpr int kDqk = 192, kDv = 128;       // head dims of q / k and of v / out
constexpr int kRowB = 128;                 // bytes per panel row
constexpr int kRows = 64;                  // rows per streamed tile
constexpr int kPanelB = kRows * kRowB;     // 8 KiB
constexpr int kQkTileB = 3 * kPanelB;      // a K or Q tile: 24 KiB
constexpr int kVTileB = 2 * kPanelB;       // a V or dO tile: 16 KiB
constexpr int kLdsB = 2 * (kQkTileB + kVTileB);   // both double-buffered: 80 KiB
constexpr int kNTqk = kDqk / 16, kNTv = kDv / 16;     // k-steps of a product over the head dim
constexpr int kNDJqk = kDqk / 32, kNDJv = kDv / 32;   // 32-wide dim blocks of a transposed accumulator

USP_DEV int swz(int row) { return ((row & 2) << 1) | ((row >> 1) & 2) | ((row >> 3) & 1); }

// per-lane byte offsets (from the tile's first row in memory) of this wave's 2 NP pieces of an NP-panel tile; row_bytes = the
// tensor's row pitch
template <int NP> USP_DEV void stage_offsets(int (&voff)[2 * NP], int wave, int lane, int row_bytes) {
#pragma unroll
  for (int i = 0; i < 2 * NP; ++i) {
    const int piece = 2 * NP * wave + i;
    const int rr = 8 * (piece & 7) + (lane >> 3);
    voff[i] = rr * row_bytes + (piece >> 3) * kRowB + (((lane & 7) ^ swz(rr)) * 16);
  }
}
// Descriptor of the tile that starts at row `row0` of a tensor of `n_rows` rows of D values (`base` = row 0, `ss` = row pitch in
// elements): the tile offset sits in the 64-bit base, the byte count ends behind the last valid row's D values (none left: every
// lane reads 0).
template <int D> USP_DEV auto tile_rsrc(const char* base, int64_t ss, int row0, int n_rows) {
  int64_t rem = ((int64_t)(n_rows - 1 - row0) * ss + D) * 2;
  rem = rem < 0 ? 0 : (rem > 0xffffffffLL ? 0xffffffffLL : rem);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(base + (int64_t)row0 * ss * 2), 0, (int)(uint32_t)rem, 0x00020000);
}
template <int NP, class R> USP_DEV void stage_tile(R rs, USP_LDS char* tile, int wave, const int (&voff)[2 * NP]) {
#pragma unroll
  for (int i = 0; i < 2 * NP; ++i) lds_dma16(rs, tile + (2 * NP * wave + i) * 1024, voff[i]);
}

// Lane-constant parts of the read addresses.  The swizzle of a row depends on its bits 1-3, which a 32-row block or a 16-row step
// does not reach, and a k-step / dim block moves slot bits the lane part does not hold, so every address of a tile is ONE lane base
// with a constant XORed in, plus an immediate for the panel and the row block:
//   rows: row 32 blk + (lane & 31), panel t / 4, slot 2 (t % 4) + hi                     -> (rows ^ 32 (t % 4)) + immediates
//   tr:   row r16 + 8 e + 4 hi + (i >> 2), panel dj / 2, slot 4 (dj % 2) + 2 g + (i & 3) / 2, byte 8 (i & 1)
//                                                                                         -> (tr[e] ^ 64 (dj % 2)) + immediates
// (i = lane & 15, g = (lane >> 4) & 1, hi = lane >> 5).  The kernels pass the bases through an opaque asm once per tile: hipcc
// otherwise hoists the XORed addresses out of the tile loop and spills them.
struct LaneBase {
  int rows, tr[2];
  USP_DEV explicit LaneBase(int lane) {
    const int l31 = lane & 31, hi = lane >> 5, i = lane & 15, g = (lane >> 4) & 1;
    rows = l31 * kRowB + ((hi ^ swz(l31)) * 16);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int r = 8 * e + 4 * hi + (i >> 2);
      tr[e] = r * kRowB + (((2 * g + ((i & 3) >> 1)) ^ swz(r)) * 16) + (i & 1) * 8;
    }
  }
  USP_DEV void keep_opaque() { asm volatile("" : "+v"(rows), "+v"(tr[0]), "+v"(tr[1])); }
};
// A operand by rows: M index = tile row 32 blk + (lane & 31), K index = dims 16 t + 8 hi .. + 7
USP_DEV u32x4 read_rows(USP_LDS const char* tile, const LaneBase& lb, int blk, int t) {
  return *(USP_LDS const u32x4*)(tile + (t >> 2) * kPanelB + blk * 32 * kRowB + (lb.rows ^ (32 * (t & 3))));
}
// A operand transposed: M index = dims 32 dj + (lane & 31), K index k = 8 hi + e <-> tile row r16 + (e & 3) + 8 (e >> 2) + 4 hi: the
// order in which a 32x32 accumulator's registers 8 ks .. 8 ks + 7 hold their M index, so a packed score block is the B operand
// as it stands.
USP_DEV u32x4 read_tr(USP_LDS const char* tile, const LaneBase& lb, int r16, int dj) {
  USP_LDS const char* at = tile + (dj >> 1) * kPanelB + r16 * kRowB;
  const u32x2 v0 = lds_read_tr16(at + (lb.tr[0] ^ (64 * (dj & 1))));
  const u32x2 v1 = lds_read_tr16(at + (lb.tr[1] ^ (64 * (dj & 1))));
  return u32x4{v0[0], v0[1], v1[0], v1[1]};
}
// M index (row of S^T, key of S) that accumulator register r of a 32x32 block holds in half-wave hi
USP_DEV int acc_m(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

}  // namespace qk192

// The launches (usp_flash_fwd.hip / usp_flash_bwd.hip hand every (192, 128) call of usp_flash_fwd_vdim / usp_flash_bwd_vdim here):
// the argument blocks are complete but for nq / nblk / n_items.  USP_OK / USP_ELAUNCH / USP_EUNSUPPORTED (a row pitch of 2^24
// elements or more).
struct FwdParams;
struct BwdParams;
int launch_fwd_qk192(const FwdParams& p, int dtype, bool causal, hipStream_t st);
int launch_dq_qk192(const BwdParams& p, int dtype, bool causal, hipStream_t st);
int launch_dkdv_qk192(const BwdParams& p, int dtype, bool causal, hipStream_t st);

}  // namespace usp
