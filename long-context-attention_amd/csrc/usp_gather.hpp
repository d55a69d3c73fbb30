// The gathered-key forward (usp_flash_fwd_gather.hip): its argument block, its tile image and the index maps of a tile whose 64 rows
// come from 64 arbitrary sequence positions.
//   tile    64 rows x D 16-bit values (D = 64 | 128), row-major, a row = D / 8 slots of 16 bytes; K and V share the image, because
//           K is read by rows (A operand of S^T = K Q^T) and V transposed (ds_read_b64_tr_b16: A operand of O^T += V^T P^T)
//   swizzle logical slot s of row r sits in physical slot s ^ swz(r).  D = 128 (one row per 256-byte bank row): the head-dim-256
//           image's map, the 16 rows of a ds_read_b128 group differ in all four bits, the 4 rows of a transposed read in bits 2-3.
//           D = 64 (two rows per bank row, the row's parity picks the half): the bit reversal of (r >> 1) & 7 -- the 8 rows of one
//           parity take 8 distinct slots, the 4 rows of a transposed read differ in parity and in bit 2.
//   fill    LDS-DMA, 1 KiB = 1024 / (2 D) rows per wave instruction; wave w of 4 fills rows 16 w .. 16 w + 15.  The lane that lands on
//           physical slot p of tile row r fetches 16 bytes at  entry(r) * row pitch + 16 * (p ^ swz(r)):  the row's sequence position
//           is a PER-LANE term of the offset, so a gathered tile costs the instructions of a contiguous one.  An absent entry gets an
//           offset behind the descriptor's byte count and reads zeros.
// MFMA operand layouts: usp_common.hpp.
#pragma once
#include "usp_fwd_params.hpp"

namespace usp {

// Kernel arguments of the gathered instantiations only; every other kernel keeps its argument block and machine code.
struct FwdArgsGather : FwdParams {
  const int* kidx;                      // int32: the list of (b, h) starts at kidx + b * kidx_sb + h * kidx_sh, n_idx entries, ascending
  int64_t kidx_sb, kidx_sh;
  int n_idx;
  int win_on, left;                     // the band: row i also sees keys d_i - left .. d_i (left clamped to Sk by the host)
  int k_bytes, v_bytes;                 // extent of one (batch, kv head) plane of k / v from its first row, in bytes (< 2^31)
};
int launch_fwd_gather(const FwdArgsGather& p, int D, int dtype, hipStream_t st);

namespace gather {

constexpr int kRows = 64;                      // rows (keys) per tile
constexpr int kRing = 4;                       // index tiles in LDS (256 bytes each)

template <int D> struct Img {
  static constexpr int kRowB = 2 * D;          // bytes per tile row
  static constexpr int kSPR = D / 8;           // 16-byte slots per row
  static constexpr int kTileB = kRows * kRowB;
  static constexpr int kNT = D / 16;           // k-steps of a product over the head dim
  static constexpr int kNDJ = D / 32;          // 32-wide dim blocks of a transposed accumulator
  static constexpr int kRPP = 64 / kSPR;       // rows per 1 KiB piece
  static constexpr int kNP = 16 / kRPP;        // pieces per wave and tile
  static USP_DEV int swz(int r) {
    if (D == 128) return ((r & 3) << 2) | ((r >> 2) & 3);
    return ((r & 2) << 1) | ((r >> 1) & 2) | ((r >> 3) & 1);
  }
  // piece i of wave `wave`: the tile row this lane fetches, and the byte offset inside the source row it fetches from
  static USP_DEV int piece_row(int wave, int lane, int i) { return 16 * wave + kRPP * i + lane / kSPR; }
  static USP_DEV int piece_col(int lane, int row) { return ((lane % kSPR) ^ swz(row)) * 16; }
};

// Lane-constant parts of the read addresses (as usp_d256.hpp: one lane base with a constant XORed in per k-step / dim block):
//   rows: row 32 blk + (lane & 31), slot 2 t + hi                                     -> blk * 32 rows + (rows ^ 32 t)
//   tr:   row r16 + 8 e + 4 hi + (i >> 2), slot 4 dj + 2 g + (i & 3) / 2, byte 8 (i & 1) -> r16 rows + (tr[e] ^ 64 dj)
template <int D> struct LaneBase {
  using I = Img<D>;
  int rows, tr[2];
  USP_DEV explicit LaneBase(int lane) {
    const int l31 = lane & 31, hi = lane >> 5, i = lane & 15, g = (lane >> 4) & 1;
    rows = l31 * I::kRowB + ((hi ^ I::swz(l31 & 15)) * 16);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int r = 8 * e + 4 * hi + (i >> 2);
      tr[e] = r * I::kRowB + (((2 * g + ((i & 3) >> 1)) ^ I::swz(r)) * 16) + (i & 1) * 8;
    }
  }
  USP_DEV void keep_opaque() { asm volatile("" : "+v"(rows), "+v"(tr[0]), "+v"(tr[1])); }
  // A operand by rows: M index = tile row 32 blk + (lane & 31), K index = dims 16 t + 8 hi .. + 7
  USP_DEV u32x4 read_rows(USP_LDS const char* tile, int blk, int t) const {
    return *(USP_LDS const u32x4*)(tile + blk * 32 * I::kRowB + (rows ^ (32 * t)));
  }
  // A operand transposed: M index = dims 32 dj + (lane & 31), K index k = 8 hi + e <-> tile row r16 + (e & 3) + 8 (e >> 2) + 4 hi: the
  // order in which a 32x32 accumulator's registers hold their M index, so a packed score block is the B operand as it stands
  USP_DEV u32x4 read_tr(USP_LDS const char* tile, int r16, int dj) const {
    const u32x2 v0 = lds_read_tr16(tile + r16 * I::kRowB + (tr[0] ^ (64 * dj)));
    const u32x2 v1 = lds_read_tr16(tile + r16 * I::kRowB + (tr[1] ^ (64 * dj)));
    return u32x4{v0[0], v0[1], v1[0], v1[1]};
  }
};
// M index (row of S^T, key column of the tile) that accumulator register r of a 32x32 block holds in half-wave hi
USP_DEV int acc_m(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

}  // namespace gather
}  // namespace usp
