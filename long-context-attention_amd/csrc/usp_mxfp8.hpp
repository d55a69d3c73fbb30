// The scale operands of the MXFP8 forward (usp_flash_fwd_mxfp8.hip: e4m3 q, k, v with one E8M0 byte per OCP MX block of 32 elements)
// on v_mfma_scale_f32_32x32x64_f8f6f4.  Tile image, LDS-DMA fill, swizzle and BOTH operand byte orders are those of usp_fp8.hpp,
// unchanged -- because of what the instruction does with its 64 k indices, probed on the device once (one MFMA per case, operands
// of ones, distinct scale bytes in every lane and byte; every one of the 1024 results of each case compared):
//   data    a lane holds 8 registers = 32 bytes of row (lane & 31).  Registers 0-3 of BOTH half-waves are the 32 k indices of
//           k-block 0, registers 4-7 of both half-waves those of k-block 1: the 32 values of one block of one row are split over
//           lanes l and l + 32, 16 bytes each.  (A lane's 32 bytes are NOT one block, whatever a reading of "one scale per lane"
//           suggests: a non-zero only in registers 4-7 of lanes 0-31 is scaled by the scale bytes of lanes 32-63.)
//   scales  the scale register of lane l holds the E8M0 byte (value 2^(byte - 127)) of (row l & 31, k-block l >> 5), for A and for B
//           alike; op_sel n (the builtin's opsel argument, 0 .. 3) takes byte n of that register, the same n in every lane.
// usp_fp8.hpp's orders put whole 32-element blocks on the k-blocks already:
//   S^T = K Q^T     byte j of half-wave hi of k-step t is dim 64 t + 32 (j >> 4) + 16 hi + (j & 15): registers 0-3 lie in the MX block
//                   2 t of the head dim, registers 4-7 in block 2 t + 1.  Lane (l31, hi) supplies the byte of (row l31, block 2 t + hi):
//                   of key 32 kb + l31 for A, of query row 32 rq + l31 for B.  A row's four bytes are ONE 32-bit load, permuted
//                   (scale_pair) so that byte t of the register is block 2 t + hi: op_sel = t.
//   O^T += V^T P^T  byte j of half-wave hi is key 32 (j >> 4) + acc_m(j & 15, hi) of the tile: registers 0-3 lie in the tile's first
//                   32-key block, registers 4-7 in its second.  Lane (l31, hi) supplies v_scale[2 tile + hi][32 dj + l31] for A: four
//                   byte loads a tile packed (scale_quad) so that byte dj serves dim block dj: op_sel = dj.  B is P: the constant 127.
// Neither v_permlane32_swap nor another transposing-read order is needed: the S^T accumulators' key order IS block-major.
// Scale fetches run one tile ahead of their use, from global memory into registers (4 bytes per key and 4 per lane for V: nothing
// worth an LDS round trip).  Indices behind the tensor's end are clamped to its last key / block: those keys' data read as zero
// through the tile descriptor, so any finite scale serves.
#pragma once
#include "usp_fp8.hpp"

namespace usp {
namespace mx {

constexpr int kBlock = 32;                 // elements of one MX block
constexpr int kOne = 127;                  // the E8M0 byte of 2^0

template <int SEL_A, int SEL_B> USP_DEV f32x16 mfma(i32x8 a, i32x8 b, f32x16 c, int scale_a, int scale_b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, SEL_A, scale_a, SEL_B, scale_b);
#else
  return c;
#endif
}
// the four block bytes of a q / k row (block i in byte i) -> byte t = block 2 t + hi
USP_DEV int scale_pair(uint32_t row4, int hi) {
  const uint32_t s = row4 >> (8 * hi);
  return (int)((s & 0xffu) | ((s >> 8) & 0xff00u));
}
USP_DEV int scale_quad(const int (&b)[4]) { return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24); }

}  // namespace mx

// The launch (usp_flash_fwd.hip hands every usp_flash_fwd_mxfp8 call here): as launch_fwd_fp8, with the three scale tensors (strides
// in bytes, already checked) in place of the descales.
struct FwdParams;
int launch_fwd_mxfp8(const FwdParams& p, const usp_tensor& q_scale, const usp_tensor& k_scale, const usp_tensor& v_scale,
                     int out_dtype, bool causal, hipStream_t st);

}  // namespace usp
