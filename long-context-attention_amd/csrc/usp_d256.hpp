// The tile image of the head-dim-256 kernels (usp_flash_fwd_d256.hip, usp_flash_bwd_d256.hip): ONE image for every streamed
// tensor (K, V, Q, dO), because every one of them is read both ways -- by rows (A operand of a score product) and transposed
// (A operand of an accumulator product: ds_read_b64_tr_b16).
//   tile    64 rows x 256 16-bit values = 64 x 512 bytes, row-major; a row is 32 slots of 16 bytes
//   swizzle logical slot s of row r sits in physical slot s ^ swz(r), swz(r) = ((r & 3) << 2) | ((r >> 2) & 3): the 16 rows a
//           16-lane group of ds_read_b128 touches differ in all four low bits (16 distinct slots of the 256-byte bank row), the 4
//           rows a transposed read touches differ in bits 2-3 (four distinct 64-byte quarters)
//   fill    LDS-DMA, 1 KiB = 2 rows per wave instruction; wave w of 4 fills rows 16 w .. 16 w + 15 in 8 pieces.  The swizzle is
//           applied on the SOURCE side: the lane landing on physical slot p of row r fetches logical slot p ^ swz(r).  Rows
//           behind the tensor's last one read as zero through the descriptor's byte count.
// MFMA operand layouts: usp_common.hpp.
#pragma once
#include "usp_common.hpp"

namespace usp {
namespace d256 {

constexpr int kD = 256;
constexpr int kRowB = 2 * kD;              // bytes per tile row
constexpr int kRows = 64;                  // rows per streamed tile
constexpr int kTileB = kRows * kRowB;      // 32 KiB
constexpr int kNT = kD / 16;               // k-steps of a product over the head dim
constexpr int kNDJ = kD / 32;              // 32-wide dim blocks of a transposed accumulator

USP_DEV int swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// per-lane byte offsets (from the tile's first row in memory) of this wave's 8 pieces; row_bytes = the tensor's row pitch
USP_DEV void stage_offsets(int (&voff)[8], int wave, int lane, int row_bytes) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int rr = 16 * wave + 2 * i + (lane >> 5);
    voff[i] = rr * row_bytes + (((lane & 31) ^ swz(rr)) * 16);
  }
}
// Descriptor of the tile that starts at row `row0` of a tensor of `n_rows` rows (`base` = row 0, `ss` = row pitch in elements): the
// tile offset sits in the 64-bit base, the byte count ends behind the last valid row's 256 values (none left: every lane reads 0).
USP_DEV auto tile_rsrc(const char* base, int64_t ss, int row0, int n_rows) {
  int64_t rem = ((int64_t)(n_rows - 1 - row0) * ss + kD) * 2;
  rem = rem < 0 ? 0 : (rem > 0xffffffffLL ? 0xffffffffLL : rem);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(base + (int64_t)row0 * ss * 2), 0, (int)(uint32_t)rem, 0x00020000);
}
template <class R> USP_DEV void stage_tile(R rs, USP_LDS char* tile, int wave, const int (&voff)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) lds_dma16(rs, tile + (16 * wave + 2 * i) * kRowB, voff[i]);
}

// Lane-constant parts of the read addresses.  The swizzle of a row depends on its low four bits and a k-step / dim block moves
// slot bits the lane part does not reach, so every address of a tile is ONE lane base with a constant XORed in (plus an immediate):
//   rows: row 32 blk + (lane & 31), slot 2 t + hi                    -> blk * 16 KiB + (rows ^ 32 t)
//   tr:   row r16 + 8 e + 4 hi + (i >> 2), slot 4 dj + 2 g + (i & 3) / 2, byte 8 (i & 1)   -> r16 * 512 + (tr[e] ^ 64 dj)
// (i = lane & 15, g = (lane >> 4) & 1, hi = lane >> 5).  The kernels pass the bases through an opaque asm once per tile: hipcc
// otherwise hoists the 16 + 16 XORed addresses out of the tile loop and spills them.
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
  return *(USP_LDS const u32x4*)(tile + blk * 32 * kRowB + (lb.rows ^ (32 * t)));
}
// A operand transposed: M index = dims 32 dj + (lane & 31), K index k = 8 hi + e <-> tile row r16 + (e & 3) + 8 (e >> 2) + 4 hi: the
// order in which a 32x32 accumulator's registers 8 ks .. 8 ks + 7 hold their M index, so a packed score block is the B operand
// as it stands.
USP_DEV u32x4 read_tr(USP_LDS const char* tile, const LaneBase& lb, int r16, int dj) {
  const u32x2 v0 = lds_read_tr16(tile + r16 * kRowB + (lb.tr[0] ^ (64 * dj)));
  const u32x2 v1 = lds_read_tr16(tile + r16 * kRowB + (lb.tr[1] ^ (64 * dj)));
  return u32x4{v0[0], v0[1], v1[0], v1[1]};
}
// M index (row of S^T, key of S) that accumulator register r of a 32x32 block holds in half-wave hi
USP_DEV int acc_m(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

}  // namespace d256

// The launches (usp_flash_fwd.hip / usp_flash_bwd.hip hand every D == 256 call here): the argument blocks are complete but for
// nq / nblk / n_items.  USP_OK / USP_ELAUNCH / USP_EUNSUPPORTED (a row pitch of 2^24 elements or more).
struct FwdParams;
struct BwdParams;
int launch_fwd_d256(const FwdParams& p, int dtype, bool causal, hipStream_t st);
int launch_dq_d256(const BwdParams& p, int dtype, bool causal, hipStream_t st);
int launch_dkdv_d256(const BwdParams& p, int dtype, bool causal, hipStream_t st);

}  // namespace usp
