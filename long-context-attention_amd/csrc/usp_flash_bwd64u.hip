// Blockwise flash-attention backward for gfx950, dK/dV launch, ONE WAVE PER SIMD, ONE PROGRAM FOR ALL FOUR WAVES ("unified").
// C ABI: usp_flash_bwd (include/usp_hip.h); the 256-key-item form of usp_flash_bwd64.hip's kernel (USP_DKDV_KEYS256).
//
// usp_flash_bwd64.hip splits a 64-key slice over two waves (role A: S, P, dV; role B: dP, dS, dK): P crosses LDS, B runs a tile
// behind A, the two unequal roles meet at one barrier per 64 MFMAs, and a 128-key item re-streams Q / dO.  Here a wave does
// all four products for its own 64 keys:
//   workgroup = 4 waves = 256 keys of one (batch, kv head[, run of query heads, cut]); wave w owns keys own0 + 64 w ...
//   a[0:255]   dV^T and dK^T accumulators of the wave, 2 tensors x 2 key blocks x 4 dim tiles      (asm MFMAs, "+a")
//   v[0:127]   K and V fragments of the wave's 64 keys: B operands of the S / dP chains (the accumulator file is full)
//   v[...]     per 32-row SLICE of the streamed tile: S (32) and dP (32), started from -lse / scale and -delta, packed P (16)
//              and packed dS (16), a few LDS fragments in flight
// P and dS never touch LDS: the chain's accumulator, packed, is the B operand of the gradient MFMA (the k-step order of the
// gradient MFMAs is the order the S accumulator holds rows, as in the other kernels).  A tile (64 rows of Q + 64 of dO, 3-deep
// LDS ring, no P area) is two slices of 64 MFMA slots:  S chain | dP chain | dV | dK  (16 each); P's elements stream through
// the dP chain's slots, dS's through the dV slots and the head of the dK slots; LDS fragments are read a few slots ahead of the
// MFMA that takes them.  Every wave stages one 16-row group of Q and one of dO per tile (8 LDS-DMA pieces per 128 MFMAs), the
// statistics wave works as in usp_flash_bwd64.hip, one barrier per tile.
// What is NOT arithmetic is kept off the issue port, which is what bounds this kernel (profiles/dkdv64u_diet.txt):
//   addresses   a swizzled LDS address is formed once per slice and serves every fragment that differs from it by an immediate:
//               the seven kr ^ (32 j) of the Q rows serve the dO rows (+ TILEB), the seven tr ^ (64 dj [+ 32]) of dO^T serve its second
//               k-step and both of Q^T's -- 28 v_xor per tile, not 56.  They live where other tile state is dead (see rd()).
//   constants   the rows' constants of a chain are the same for both key blocks: ONE read, into key block 1's accumulator; key block
//               0's first MFMA takes them from there as SrcC with its own accumulator as D.  No second read, no copy, and so no
//               VALU write in front of an MFMA's SrcC: the plain loop's chains start without wait states.
//   staging     the two LDS-DMA descriptors ARE the tile cursors (stepped in place, 3 scalar instructions each), a piece's row step
//               rides its lanes' offsets instead of a scalar offset, the ring position is a byte offset, and the statistics rows'
//               validity is recomputed where it is used instead of being carried as a lane mask.
// Arithmetic is that kernel's, step for step (dS = the 16-bit P that feeds dV, unpacked, times (dP - delta); same tile, half and
// k-step order): at equal dkdv_heads, dK and dV are bit-identical to it for uncut launches and for cut launches without a causal
// bound (a cut causal launch cuts a block's second 128 keys at other query tiles than the 128-key item: tests/test_gpu_dkdv256.py).
#ifdef USP_B64U_TIMING
#define USP_TIMING
#endif
#include "usp_bwd_params.hpp"
#include "usp_host.hpp"
#include "usp_mfma64.hpp"
#include <utility>

namespace usp {

// slots of a slice's element streams (first, one past last): P = exp2(S c) rides [PE0, PE1), dS = P (dP - delta) [SE0, SE1).
// The S chain ends at slot 16, the dP chain at 32; dV of k-step k2 starts at 32 + 8 k2, dK at 48 + 8 k2.  (-D overrides: sweeps only.)
#ifndef USP_B64U_PE0
#define USP_B64U_PE0 17
#endif
#ifndef USP_B64U_PE1
#define USP_B64U_PE1 33
#endif
#ifndef USP_B64U_SE0
#define USP_B64U_SE0 33
#endif
#ifndef USP_B64U_SE1
#define USP_B64U_SE1 55
#endif
#ifndef USP_B64U_LA
#define USP_B64U_LA 3
#endif
constexpr int kU_PE0 = USP_B64U_PE0, kU_PE1 = USP_B64U_PE1, kU_SE0 = USP_B64U_SE0, kU_SE1 = USP_B64U_SE1;
constexpr int kU_LA = USP_B64U_LA;        // LDS fragments are requested this many fragments (two slots each) ahead of their first MFMA

// The accumulator file is owned by hand: the wave's 16 accumulators (index 8 tensor + 4 key block + dim tile; tensor 0 = dV, 1 = dK)
// ARE a[0:255], named in the asm text and never C++ values -- as values, with the file full, hipcc gives them VGPR homes and
// copies them around every MFMA (32 v_accvgpr moves per MFMA and scratch traffic in the loop; physical-register CONSTRAINTS
// crash this hipcc's machine scheduler; profiles/dkdv_unified.txt).  hipcc itself allocates no AGPR in this kernel (the clobber
// lists keep them out of its reach as spill slots; the build's census shows no v_accvgpr instruction but the epilogue's reads).
// The index is a constant after unrolling; the dead cases fold away.  X(index, tuple, the 16 reads, clobbers...)
#define USP_U_ACC16(X) \
  X(0, "a[0:15]", "v_accvgpr_read_b32 %0, a0\n\tv_accvgpr_read_b32 %1, a1\n\tv_accvgpr_read_b32 %2, a2\n\tv_accvgpr_read_b32 %3, a3\n\tv_accvgpr_read_b32 %4, a4\n\tv_accvgpr_read_b32 %5, a5\n\tv_accvgpr_read_b32 %6, a6\n\tv_accvgpr_read_b32 %7, a7\n\tv_accvgpr_read_b32 %8, a8\n\tv_accvgpr_read_b32 %9, a9\n\tv_accvgpr_read_b32 %10, a10\n\tv_accvgpr_read_b32 %11, a11\n\tv_accvgpr_read_b32 %12, a12\n\tv_accvgpr_read_b32 %13, a13\n\tv_accvgpr_read_b32 %14, a14\n\tv_accvgpr_read_b32 %15, a15", "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15") \
  X(1, "a[16:31]", "v_accvgpr_read_b32 %0, a16\n\tv_accvgpr_read_b32 %1, a17\n\tv_accvgpr_read_b32 %2, a18\n\tv_accvgpr_read_b32 %3, a19\n\tv_accvgpr_read_b32 %4, a20\n\tv_accvgpr_read_b32 %5, a21\n\tv_accvgpr_read_b32 %6, a22\n\tv_accvgpr_read_b32 %7, a23\n\tv_accvgpr_read_b32 %8, a24\n\tv_accvgpr_read_b32 %9, a25\n\tv_accvgpr_read_b32 %10, a26\n\tv_accvgpr_read_b32 %11, a27\n\tv_accvgpr_read_b32 %12, a28\n\tv_accvgpr_read_b32 %13, a29\n\tv_accvgpr_read_b32 %14, a30\n\tv_accvgpr_read_b32 %15, a31", "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31") \
  X(2, "a[32:47]", "v_accvgpr_read_b32 %0, a32\n\tv_accvgpr_read_b32 %1, a33\n\tv_accvgpr_read_b32 %2, a34\n\tv_accvgpr_read_b32 %3, a35\n\tv_accvgpr_read_b32 %4, a36\n\tv_accvgpr_read_b32 %5, a37\n\tv_accvgpr_read_b32 %6, a38\n\tv_accvgpr_read_b32 %7, a39\n\tv_accvgpr_read_b32 %8, a40\n\tv_accvgpr_read_b32 %9, a41\n\tv_accvgpr_read_b32 %10, a42\n\tv_accvgpr_read_b32 %11, a43\n\tv_accvgpr_read_b32 %12, a44\n\tv_accvgpr_read_b32 %13, a45\n\tv_accvgpr_read_b32 %14, a46\n\tv_accvgpr_read_b32 %15, a47", "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47") \
  X(3, "a[48:63]", "v_accvgpr_read_b32 %0, a48\n\tv_accvgpr_read_b32 %1, a49\n\tv_accvgpr_read_b32 %2, a50\n\tv_accvgpr_read_b32 %3, a51\n\tv_accvgpr_read_b32 %4, a52\n\tv_accvgpr_read_b32 %5, a53\n\tv_accvgpr_read_b32 %6, a54\n\tv_accvgpr_read_b32 %7, a55\n\tv_accvgpr_read_b32 %8, a56\n\tv_accvgpr_read_b32 %9, a57\n\tv_accvgpr_read_b32 %10, a58\n\tv_accvgpr_read_b32 %11, a59\n\tv_accvgpr_read_b32 %12, a60\n\tv_accvgpr_read_b32 %13, a61\n\tv_accvgpr_read_b32 %14, a62\n\tv_accvgpr_read_b32 %15, a63", "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63") \
  X(4, "a[64:79]", "v_accvgpr_read_b32 %0, a64\n\tv_accvgpr_read_b32 %1, a65\n\tv_accvgpr_read_b32 %2, a66\n\tv_accvgpr_read_b32 %3, a67\n\tv_accvgpr_read_b32 %4, a68\n\tv_accvgpr_read_b32 %5, a69\n\tv_accvgpr_read_b32 %6, a70\n\tv_accvgpr_read_b32 %7, a71\n\tv_accvgpr_read_b32 %8, a72\n\tv_accvgpr_read_b32 %9, a73\n\tv_accvgpr_read_b32 %10, a74\n\tv_accvgpr_read_b32 %11, a75\n\tv_accvgpr_read_b32 %12, a76\n\tv_accvgpr_read_b32 %13, a77\n\tv_accvgpr_read_b32 %14, a78\n\tv_accvgpr_read_b32 %15, a79", "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79") \
  X(5, "a[80:95]", "v_accvgpr_read_b32 %0, a80\n\tv_accvgpr_read_b32 %1, a81\n\tv_accvgpr_read_b32 %2, a82\n\tv_accvgpr_read_b32 %3, a83\n\tv_accvgpr_read_b32 %4, a84\n\tv_accvgpr_read_b32 %5, a85\n\tv_accvgpr_read_b32 %6, a86\n\tv_accvgpr_read_b32 %7, a87\n\tv_accvgpr_read_b32 %8, a88\n\tv_accvgpr_read_b32 %9, a89\n\tv_accvgpr_read_b32 %10, a90\n\tv_accvgpr_read_b32 %11, a91\n\tv_accvgpr_read_b32 %12, a92\n\tv_accvgpr_read_b32 %13, a93\n\tv_accvgpr_read_b32 %14, a94\n\tv_accvgpr_read_b32 %15, a95", "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95") \
  X(6, "a[96:111]", "v_accvgpr_read_b32 %0, a96\n\tv_accvgpr_read_b32 %1, a97\n\tv_accvgpr_read_b32 %2, a98\n\tv_accvgpr_read_b32 %3, a99\n\tv_accvgpr_read_b32 %4, a100\n\tv_accvgpr_read_b32 %5, a101\n\tv_accvgpr_read_b32 %6, a102\n\tv_accvgpr_read_b32 %7, a103\n\tv_accvgpr_read_b32 %8, a104\n\tv_accvgpr_read_b32 %9, a105\n\tv_accvgpr_read_b32 %10, a106\n\tv_accvgpr_read_b32 %11, a107\n\tv_accvgpr_read_b32 %12, a108\n\tv_accvgpr_read_b32 %13, a109\n\tv_accvgpr_read_b32 %14, a110\n\tv_accvgpr_read_b32 %15, a111", "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111") \
  X(7, "a[112:127]", "v_accvgpr_read_b32 %0, a112\n\tv_accvgpr_read_b32 %1, a113\n\tv_accvgpr_read_b32 %2, a114\n\tv_accvgpr_read_b32 %3, a115\n\tv_accvgpr_read_b32 %4, a116\n\tv_accvgpr_read_b32 %5, a117\n\tv_accvgpr_read_b32 %6, a118\n\tv_accvgpr_read_b32 %7, a119\n\tv_accvgpr_read_b32 %8, a120\n\tv_accvgpr_read_b32 %9, a121\n\tv_accvgpr_read_b32 %10, a122\n\tv_accvgpr_read_b32 %11, a123\n\tv_accvgpr_read_b32 %12, a124\n\tv_accvgpr_read_b32 %13, a125\n\tv_accvgpr_read_b32 %14, a126\n\tv_accvgpr_read_b32 %15, a127", "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127") \
  X(8, "a[128:143]", "v_accvgpr_read_b32 %0, a128\n\tv_accvgpr_read_b32 %1, a129\n\tv_accvgpr_read_b32 %2, a130\n\tv_accvgpr_read_b32 %3, a131\n\tv_accvgpr_read_b32 %4, a132\n\tv_accvgpr_read_b32 %5, a133\n\tv_accvgpr_read_b32 %6, a134\n\tv_accvgpr_read_b32 %7, a135\n\tv_accvgpr_read_b32 %8, a136\n\tv_accvgpr_read_b32 %9, a137\n\tv_accvgpr_read_b32 %10, a138\n\tv_accvgpr_read_b32 %11, a139\n\tv_accvgpr_read_b32 %12, a140\n\tv_accvgpr_read_b32 %13, a141\n\tv_accvgpr_read_b32 %14, a142\n\tv_accvgpr_read_b32 %15, a143", "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143") \
  X(9, "a[144:159]", "v_accvgpr_read_b32 %0, a144\n\tv_accvgpr_read_b32 %1, a145\n\tv_accvgpr_read_b32 %2, a146\n\tv_accvgpr_read_b32 %3, a147\n\tv_accvgpr_read_b32 %4, a148\n\tv_accvgpr_read_b32 %5, a149\n\tv_accvgpr_read_b32 %6, a150\n\tv_accvgpr_read_b32 %7, a151\n\tv_accvgpr_read_b32 %8, a152\n\tv_accvgpr_read_b32 %9, a153\n\tv_accvgpr_read_b32 %10, a154\n\tv_accvgpr_read_b32 %11, a155\n\tv_accvgpr_read_b32 %12, a156\n\tv_accvgpr_read_b32 %13, a157\n\tv_accvgpr_read_b32 %14, a158\n\tv_accvgpr_read_b32 %15, a159", "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159") \
  X(10, "a[160:175]", "v_accvgpr_read_b32 %0, a160\n\tv_accvgpr_read_b32 %1, a161\n\tv_accvgpr_read_b32 %2, a162\n\tv_accvgpr_read_b32 %3, a163\n\tv_accvgpr_read_b32 %4, a164\n\tv_accvgpr_read_b32 %5, a165\n\tv_accvgpr_read_b32 %6, a166\n\tv_accvgpr_read_b32 %7, a167\n\tv_accvgpr_read_b32 %8, a168\n\tv_accvgpr_read_b32 %9, a169\n\tv_accvgpr_read_b32 %10, a170\n\tv_accvgpr_read_b32 %11, a171\n\tv_accvgpr_read_b32 %12, a172\n\tv_accvgpr_read_b32 %13, a173\n\tv_accvgpr_read_b32 %14, a174\n\tv_accvgpr_read_b32 %15, a175", "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175") \
  X(11, "a[176:191]", "v_accvgpr_read_b32 %0, a176\n\tv_accvgpr_read_b32 %1, a177\n\tv_accvgpr_read_b32 %2, a178\n\tv_accvgpr_read_b32 %3, a179\n\tv_accvgpr_read_b32 %4, a180\n\tv_accvgpr_read_b32 %5, a181\n\tv_accvgpr_read_b32 %6, a182\n\tv_accvgpr_read_b32 %7, a183\n\tv_accvgpr_read_b32 %8, a184\n\tv_accvgpr_read_b32 %9, a185\n\tv_accvgpr_read_b32 %10, a186\n\tv_accvgpr_read_b32 %11, a187\n\tv_accvgpr_read_b32 %12, a188\n\tv_accvgpr_read_b32 %13, a189\n\tv_accvgpr_read_b32 %14, a190\n\tv_accvgpr_read_b32 %15, a191", "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191") \
  X(12, "a[192:207]", "v_accvgpr_read_b32 %0, a192\n\tv_accvgpr_read_b32 %1, a193\n\tv_accvgpr_read_b32 %2, a194\n\tv_accvgpr_read_b32 %3, a195\n\tv_accvgpr_read_b32 %4, a196\n\tv_accvgpr_read_b32 %5, a197\n\tv_accvgpr_read_b32 %6, a198\n\tv_accvgpr_read_b32 %7, a199\n\tv_accvgpr_read_b32 %8, a200\n\tv_accvgpr_read_b32 %9, a201\n\tv_accvgpr_read_b32 %10, a202\n\tv_accvgpr_read_b32 %11, a203\n\tv_accvgpr_read_b32 %12, a204\n\tv_accvgpr_read_b32 %13, a205\n\tv_accvgpr_read_b32 %14, a206\n\tv_accvgpr_read_b32 %15, a207", "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207") \
  X(13, "a[208:223]", "v_accvgpr_read_b32 %0, a208\n\tv_accvgpr_read_b32 %1, a209\n\tv_accvgpr_read_b32 %2, a210\n\tv_accvgpr_read_b32 %3, a211\n\tv_accvgpr_read_b32 %4, a212\n\tv_accvgpr_read_b32 %5, a213\n\tv_accvgpr_read_b32 %6, a214\n\tv_accvgpr_read_b32 %7, a215\n\tv_accvgpr_read_b32 %8, a216\n\tv_accvgpr_read_b32 %9, a217\n\tv_accvgpr_read_b32 %10, a218\n\tv_accvgpr_read_b32 %11, a219\n\tv_accvgpr_read_b32 %12, a220\n\tv_accvgpr_read_b32 %13, a221\n\tv_accvgpr_read_b32 %14, a222\n\tv_accvgpr_read_b32 %15, a223", "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223") \
  X(14, "a[224:239]", "v_accvgpr_read_b32 %0, a224\n\tv_accvgpr_read_b32 %1, a225\n\tv_accvgpr_read_b32 %2, a226\n\tv_accvgpr_read_b32 %3, a227\n\tv_accvgpr_read_b32 %4, a228\n\tv_accvgpr_read_b32 %5, a229\n\tv_accvgpr_read_b32 %6, a230\n\tv_accvgpr_read_b32 %7, a231\n\tv_accvgpr_read_b32 %8, a232\n\tv_accvgpr_read_b32 %9, a233\n\tv_accvgpr_read_b32 %10, a234\n\tv_accvgpr_read_b32 %11, a235\n\tv_accvgpr_read_b32 %12, a236\n\tv_accvgpr_read_b32 %13, a237\n\tv_accvgpr_read_b32 %14, a238\n\tv_accvgpr_read_b32 %15, a239", "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239") \
  X(15, "a[240:255]", "v_accvgpr_read_b32 %0, a240\n\tv_accvgpr_read_b32 %1, a241\n\tv_accvgpr_read_b32 %2, a242\n\tv_accvgpr_read_b32 %3, a243\n\tv_accvgpr_read_b32 %4, a244\n\tv_accvgpr_read_b32 %5, a245\n\tv_accvgpr_read_b32 %6, a246\n\tv_accvgpr_read_b32 %7, a247\n\tv_accvgpr_read_b32 %8, a248\n\tv_accvgpr_read_b32 %9, a249\n\tv_accvgpr_read_b32 %10, a250\n\tv_accvgpr_read_b32 %11, a251\n\tv_accvgpr_read_b32 %12, a252\n\tv_accvgpr_read_b32 %13, a253\n\tv_accvgpr_read_b32 %14, a254\n\tv_accvgpr_read_b32 %15, a255", "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255")
template <int DT> struct MU;
#if defined(__HIP_DEVICE_COMPILE__)
#define USP_MU_ACC(i, tup, rd, ...) case i: asm volatile(USP_MU_MN " " tup ", %0, %1, " tup : : "v"(a), "v"(b) : __VA_ARGS__); break;
#define USP_MU_ZERO(i, tup, rd, ...) case i: asm volatile(USP_MU_MN " " tup ", %0, %0, 0" : : "v"(z) : __VA_ARGS__); break;
#define USP_MU_BODY                                                                                                    \
  /* chain step: C/D = S or dP (arch VGPRs, started from the rows' constants), A = streamed row fragment, B = resident fragment */ \
  template <bool SAFE = false> static USP_DEV void chain(f32x16& s, const u32x4& a, const u32x4& b) {                   \
    if (SAFE) asm volatile("s_nop 1\n\t" USP_MU_MN " %0, %1, %2, %0" : "+v"(s) : "v"(a), "v"(b));                     \
    else asm volatile(USP_MU_MN " %0, %1, %2, %0" : "+v"(s) : "v"(a), "v"(b));                                          \
  }                                                                                                                     \
  /* a chain's FIRST step of key block 0: D = s, C = the rows' constants, which were read into key block 1's accumulator c */  \
  template <bool SAFE = false> static USP_DEV void chain_from(f32x16& s, const u32x4& a, const u32x4& b, const f32x16& c) { \
    if (SAFE) asm volatile("s_nop 1\n\t" USP_MU_MN " %0, %1, %2, %3" : "=&v"(s) : "v"(a), "v"(b), "v"(c));             \
    else asm volatile(USP_MU_MN " %0, %1, %2, %3" : "=&v"(s) : "v"(a), "v"(b), "v"(c));                                 \
  }                                                                                                                     \
  /* gradient accumulate: C/D = accumulator ac, A = transposed fragment, B = packed P / dS */                           \
  template <bool SAFE = false> static USP_DEV void grad(int ac, const u32x4& a, const u32x4& b) {                       \
    if (SAFE) asm volatile("s_nop 1");                                                                                  \
    switch (ac) { USP_U_ACC16(USP_MU_ACC) }                                                                             \
  }                                                                                                                     \
  /* accumulator ac = 0: z x z + 0 of a zero fragment z (the s_nop: VALU write of z -> MFMA operand) */                 \
  static USP_DEV void zero(int ac, const u32x4& z) {                                                                    \
    asm volatile("s_nop 1");                                                                                            \
    switch (ac) { USP_U_ACC16(USP_MU_ZERO) }                                                                            \
  }
#else
#define USP_MU_BODY                                                                                                    \
  template <bool SAFE = false> static USP_DEV void chain(f32x16&, const u32x4&, const u32x4&) {}                        \
  template <bool SAFE = false> static USP_DEV void chain_from(f32x16&, const u32x4&, const u32x4&, const f32x16&) {}    \
  template <bool SAFE = false> static USP_DEV void grad(int, const u32x4&, const u32x4&) {}                             \
  static USP_DEV void zero(int, const u32x4&) {}
#endif
#define USP_MU_MN "v_mfma_f32_32x32x16_bf16"
template <> struct MU<0> { USP_MU_BODY };
#undef USP_MU_MN
#define USP_MU_MN "v_mfma_f32_32x32x16_f16"
template <> struct MU<1> { USP_MU_BODY };
#undef USP_MU_MN

// accumulator ac into arch VGPRs (behind acc_settle)
USP_DEV void acc_read(int ac, f32x16& o) {
#if defined(__HIP_DEVICE_COMPILE__)
  float t[16];
#define USP_MU_READ(i, tup, rd, ...) case i: asm volatile(rd : "=v"(t[0]), "=v"(t[1]), "=v"(t[2]), "=v"(t[3]), "=v"(t[4]), "=v"(t[5]), \
    "=v"(t[6]), "=v"(t[7]), "=v"(t[8]), "=v"(t[9]), "=v"(t[10]), "=v"(t[11]), "=v"(t[12]), "=v"(t[13]), "=v"(t[14]), "=v"(t[15])); break;
  switch (ac) { USP_U_ACC16(USP_MU_READ) }
#undef USP_MU_READ
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = t[r];
#endif
}
// "XDL write -> v_accvgpr_read": the wait states hipcc cannot know it has to place
USP_DEV void acc_settle() { asm volatile("s_nop 15\n\ts_nop 3" ::: "memory"); }

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in order: the tile body is 128 slots of straight-line code, more
// than `#pragma unroll` unrolls (its size limit counts the switch cases before they fold)
template <int... I, class F> USP_DEV void static_for_seq(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F> USP_DEV void static_for(F&& f) { static_for_seq(std::make_integer_sequence<int, N>{}, f); }

USP_DEV void pin_vgpr4(u32x4& x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x));
#endif
}
// load_resident16 (usp_mfma64.hpp) into arch VGPRs
USP_DEV void load_resident16_v(u32x4 (&f0)[8], u32x4 (&f1)[8], const char* r0, const char* r1) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("global_load_dwordx4 %0, %16, off\n\tglobal_load_dwordx4 %1, %16, off offset:32\n\t"
               "global_load_dwordx4 %2, %16, off offset:64\n\tglobal_load_dwordx4 %3, %16, off offset:96\n\t"
               "global_load_dwordx4 %4, %16, off offset:128\n\tglobal_load_dwordx4 %5, %16, off offset:160\n\t"
               "global_load_dwordx4 %6, %16, off offset:192\n\tglobal_load_dwordx4 %7, %16, off offset:224\n\t"
               "global_load_dwordx4 %8, %17, off\n\tglobal_load_dwordx4 %9, %17, off offset:32\n\t"
               "global_load_dwordx4 %10, %17, off offset:64\n\tglobal_load_dwordx4 %11, %17, off offset:96\n\t"
               "global_load_dwordx4 %12, %17, off offset:128\n\tglobal_load_dwordx4 %13, %17, off offset:160\n\t"
               "global_load_dwordx4 %14, %17, off offset:192\n\tglobal_load_dwordx4 %15, %17, off offset:224\n\t"
               "s_waitcnt vmcnt(0)"
               : "=&v"(f0[0]), "=&v"(f0[1]), "=&v"(f0[2]), "=&v"(f0[3]), "=&v"(f0[4]), "=&v"(f0[5]), "=&v"(f0[6]), "=&v"(f0[7]),
                 "=&v"(f1[0]), "=&v"(f1[1]), "=&v"(f1[2]), "=&v"(f1[3]), "=&v"(f1[4]), "=&v"(f1[5]), "=&v"(f1[6]), "=&v"(f1[7])
               : "v"(r0), "v"(r1) : "memory");
#endif
}

template <int DT, bool CAUSAL>
__global__ __launch_bounds__(256, 1) void flash_bwd_dkdv64u_kernel(const BwdParams /* read through the kernarg segment */) {
  using E = Elem<DT>;
  using U = MU<DT>;
  constexpr int D = 128, OWN = 256;
  constexpr int ROWB = D * 2;
  constexpr int TILEB = kTile * ROWB;            // one streamed matrix tile (64 rows)
  constexpr int STATB = 2 * kTile * 4;           // -lse / scale + (-delta) of the tile's rows
  constexpr int BUFB = 2 * TILEB + STATB;
  constexpr int NBUF = 3;
  constexpr int NKT = D / 16, NDJ = D / 32;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  USP_LDS char* smem = lds_block_at_zero(smem_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31;
  const int hi = lane >> 5;
  typedef const __attribute__((address_space(4))) BwdParams* KArgs;
  KArgs p = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));

  // ---- lane-constant addresses (usp_flash_bwd64.hip) ----------------------------------------------------------------------
  const int dma_row = lane >> 4;
  const int dma_c8 = ((lane & 15) ^ ((lane >> 4) << 2)) * 16;
  const int q_voff = dma_row * (int)p->q_ss * 2 + dma_c8, do_voff = dma_row * (int)p->do_ss * 2 + dma_c8;
  // row read (A operand of the S / dP chains): tile row 32h + l31, logical slot 2t + hi:  ^ (32 t), + h * 32 * ROWB
  const int rd_base = l31 * ROWB + ((hi ^ tile_swz<D>(l31)) * 16);
  // transpose read (A operand of the gradient MFMAs), dim tile dj, element half e: tr_read_offset(.., dj, e) ==
  // (tr_read_offset(.., 0, 0) ^ (64 dj + 32 e)) + 2048 e -- dj and e enter the swizzled slot by XOR, e the row by 8 rows
  const int tr_base = tr_read_offset<D>(lane & 15, (lane >> 4) & 1, hi, 0, 0);

  const ItemWalk walk(p->n_items);               // persistent workgroups (usp_common.hpp)
  for (int pass = 0;; ++pass) {
  int w = walk.at(pass);
  if (w < 0) break;
  asm volatile("" : "+s"(p));
  w = walk.dealt(w, p->nblk);
  const int blk = w % p->nblk;                   // early key blocks are seen by most rows: first
  int rest = w / p->nblk;
  int g = 0, cut = 0;                            // g: which run of `gsub` query heads of the KV group this item streams
  if (p->qsplit > 1) { cut = rest % p->qsplit; rest /= p->qsplit; }
  if (p->ngrp > 1) { g = rest % p->ngrp; rest /= p->ngrp; }
  const int hkv = rest % p->Hkv, b = rest / p->Hkv;
  const int gsub = p->gsub;
  const int h0 = hkv * p->G + g * gsub;
  const int own0 = blk * OWN;
  const int off = p->causal_off;
  const int ow = own0 + wave * 64;               // first key of this wave

  // K and V fragments of this wave's 64 keys (as loaded: the S chain runs on K itself, usp_flash_bwd64.hip)
  u32x4 kf[2][NKT], vf[2][NKT];
  {
    const char *pk[2], *pv[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int orow = ow + 32 * kb + l31;
      const int orow_c = orow < p->Sk ? orow : p->Sk - 1;
      pk[kb] = p->k + 2 * (b * p->k_sb + (int64_t)orow_c * p->k_ss + hkv * p->k_sh) + 16 * hi;
      pv[kb] = p->v + 2 * (b * p->v_sb + (int64_t)orow_c * p->v_ss + hkv * p->v_sh) + 16 * hi;
    }
    load_resident16_v(kf[0], kf[1], pk[0], pk[1]);
    load_resident16_v(vf[0], vf[1], pv[0], pv[1]);
  }
  const float c2 = p->scale_log2;
  const float neg_inv_scale = -__builtin_amdgcn_rcpf(p->scale);

  // query tiles [t_begin, t_end) hold the rows that see this block's keys
  int t_end = (p->Sq + kTile - 1) / kTile;
  int t_begin = usp_first_row_tile(own0, CAUSAL, off, t_end, kTile);
  if (p->qsplit > 1) {                           // this item's cut of the query tiles [t_begin, t_end): equal runs
    const int per = usp_run_length(t_begin, t_end, p->qsplit);
    t_begin = usp_run_begin(t_begin, t_end, per, cut);
    t_end = usp_run_end(t_begin, t_end, per);
  }
  const int n_iter = t_end - t_begin;             // tiles per head

  // ---- LDS-DMA staging of the Q / dO tiles: wave w stages group w (16 rows) of Q and group w of dO ----------------------
  const int64_t tb1 = (int64_t)kTile * p->q_ss * 2, tb2 = (int64_t)kTile * p->do_ss * 2;     // bytes per tile step
  const int q_rowb = (int)p->q_ss * 2, do_rowb = (int)p->do_ss * 2;
  int lds_q = wave * 4096, lds_d = TILEB + wave * 4096;                        // LDS offsets of the groups inside a buffer
  // piece i of a group: rows 4 i .. 4 i + 3.  Its lanes' byte offsets carry the swizzle (^ 16 i) AND the row step (the instruction
  // offset 1024 i, which places the piece in LDS, counts on the global side too): lane constants, nothing scalar per piece
  int q_vo[4], do_vo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    q_vo[i] = (q_voff ^ (16 * i)) + i * (4 * q_rowb - 1024);
    do_vo[i] = (do_voff ^ (16 * i)) + i * (4 * do_rowb - 1024);
  }
  // the tile cursors ARE the descriptors (words 0-1: the 48-bit address, advanced in place; 2: the bytes the tile may read; 3: flags)
  u32x4 q_rs = u32x4{0u, 0u, 0u, 0x00020000u}, do_rs = q_rs;
  int rows_g = 0;                                // valid rows from the cursors on (<= 0: nothing left, lanes read 0)
  auto rs_move = [](u32x4& rs, int64_t by) {     // base += by, mod 2^48
    const uint64_t a = (((uint64_t)rs[1] << 32) | rs[0]) + (uint64_t)by;
    rs[0] = (uint32_t)a;
    rs[1] = (uint32_t)(a >> 32) & 0xffffu;
  };

  const float *lse_h = nullptr, *dl_h = nullptr;
  int st_row = 0;
  float st_lse = 0.f, st_delta = 0.f;
  const bool stat_wave = wave == 0;
  auto pf_head = [&](int h) {                    // base the cursors one tile IN FRONT of query head h's tile t_begin: dma_open steps first
    const uint64_t qa = (uint64_t)(p->q + 2 * (b * p->q_sb + h * p->q_sh) + (t_begin - 1) * tb1 + (int64_t)wave * 16 * q_rowb);
    const uint64_t da = (uint64_t)(p->dout + 2 * (b * p->do_sb + h * p->do_sh) + (t_begin - 1) * tb2 + (int64_t)wave * 16 * do_rowb);
    q_rs[0] = (uint32_t)qa; q_rs[1] = (uint32_t)(qa >> 32) & 0xffffu;
    do_rs[0] = (uint32_t)da; do_rs[1] = (uint32_t)(da >> 32) & 0xffffu;
    rows_g = p->Sq - (t_begin - 1) * kTile - 16 * wave;
    lse_h = p->lse + b * p->lse_sb + h * p->lse_sh;
    dl_h = p->delta + b * p->dl_sb + h * p->dl_sh;
    st_row = t_begin * kTile;
  };
  int dma_boff = 0;
  auto dma_open = [&](int boff) {                // step the cursors to the next tile, for the LDS buffer at byte offset `boff`
    rs_move(q_rs, tb1);
    rs_move(do_rs, tb2);
    rows_g -= kTile;
    const int r = (rows_g < 16 ? rows_g : 16) - 1;           // make_rsrc_rows (usp_mfma64.hpp): the group's last valid row ends the range
    const int nq = r * q_rowb + 2 * D, nd = r * do_rowb + 2 * D;
    q_rs[2] = (uint32_t)(nq > 0 ? nq : 0);
    do_rs[2] = (uint32_t)(nd > 0 ? nd : 0);
    dma_boff = boff;
  };
  auto stats_fetch = [&]() {
    if (stat_wave) {
      const int r = st_row + lane;
      const int rc = r < p->Sq ? r : p->Sq - 1;
      const float* pl = lse_h + rc;
      const float* pd = dl_h + rc;
      asm volatile("global_load_dword %0, %2, off\n\tglobal_load_dword %1, %3, off" : "=&v"(st_lse), "=&v"(st_delta) : "v"(pl), "v"(pd) : "memory");
    }
    st_row += kTile;
  };
  auto dma_piece = [&](int n) {                  // n < 4: Q piece n, else dO piece n - 4
    asm volatile("" : "+s"(lds_q), "+s"(lds_d));
    const int i = n & 3;
    if (n < 4) lds_dma16_asm(q_rs, lds_q + dma_boff, q_vo[i], 0, i);
    else lds_dma16_asm(do_rs, lds_d + dma_boff, do_vo[i], 0, i);
  };
  auto stats_store = [&](int boff) {             // behind the wave's vmcnt(0): the constants the chains START from
    if (stat_wave) {
      asm volatile("" : "+v"(st_lse), "+v"(st_delta));
      const bool st_in = st_row - kTile + lane < p->Sq;      // the row stats_fetch asked for (not carried: a lane mask across the tile is
                                                             // scalar work per tile).  Rows past the end: P = 0 (their Q / dO rows read as zero)
      const float l2 = (st_in && st_lse != USP_NEG_INF) ? st_lse * neg_inv_scale : -__builtin_inff();
      *(USP_LDS float*)(smem + boff + 2 * TILEB + 4 * lane) = l2;
      *(USP_LDS float*)(smem + boff + 2 * TILEB + 4 * kTile + 4 * lane) = st_in ? -st_delta : 0.f;
    }
  };

  // dV^T = accumulators 4 kb + dj, dK^T = 8 + 4 kb + dj: [key block][dim tile]
  u32x4 zfrag = u32x4{0u, 0u, 0u, 0u};
  asm volatile("" : "+v"(zfrag));
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int dj = 0; dj < NDJ; ++dj) { U::zero(4 * kb + dj, zfrag); U::zero(8 + 4 * kb + dj, zfrag); }

  // The tile body is STRAIGHT-LINE code and the same for every wave; the diagonal tiles -- the FIRST n_mask tiles of a causal
  // item, counted per wave: a tile none of whose rows sees the wave's keys runs fully masked, P = 0 -- run in a loop instance
  // of their own (MASK).  Every instance ends in the tile's one barrier, so the waves' barrier counts agree whatever n_mask is.
  const int n_mask = usp_masked_row_tiles(ow, CAUSAL, off, t_begin, n_iter, kTile);
  int tile_cur = t_begin, boff_a = 0;             // boff_a: byte offset of the LDS buffer that holds the current tile
USP_TM(
  uint64_t tm_body = 0, tm_drain = 0, tm_bar = 0, tm_last = __builtin_amdgcn_s_memtime();
)
  auto step = [&](auto mask_c) __attribute__((always_inline)) {
    constexpr bool MASK = decltype(mask_c)::value;
    constexpr int PE0 = kU_PE0, PE1 = kU_PE1, SE0 = kU_SE0, SE1 = kU_SE1, LA = kU_LA;
    static_assert(PE0 >= 17 && PE1 <= 40 && PE1 > PE0 && (PE0 + (PE1 - PE0 + 1) / 2) <= 31, "P of k-step 0 in front of dV");
    static_assert(SE0 >= 33 && SE1 <= 55 && SE1 > SE0 && (SE0 + (SE1 - SE0 + 1) / 2) <= 47, "dS of k-step 0 in front of dK");
    static_assert(LA >= 1 && LA <= 7, "");
    const int boff_n = boff_a + BUFB == NBUF * BUFB ? 0 : boff_a + BUFB;
    stats_fetch();
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int t = 0; t < NKT; ++t) { pin_vgpr4(kf[kb][t]); pin_vgpr4(vf[kb][t]); }
    const int s0 = tile_cur * kTile;
    USP_LDS const char* stat = smem + boff_a + 2 * TILEB + 16 * hi;
    // the buffer base goes INTO the swizzled offsets before the XOR (bases are multiples of 256, the XORs touch bits 5-7)
    int kr = rd_base + boff_a, tr = tr_base + boff_a;
    int krx[8], trx[8];                          // kr ^ (32 j); tr ^ (64 dj) at dj, tr ^ (64 dj + 32) at 4 + dj: formed ONCE per slice
    f32x16 sc[2], dp[2];                         // S / dP - delta of the slice: [key block]
    u32x4 pkp[2][2], pks[2][2];                  // packed P / dS: [key block][k-step]
    u32x4 fr[2][32];                             // the slices' LDS fragments, in MFMA order: 8 Q rows | 8 dO rows | 8 dO^T | 8 Q^T
    auto rd = [&](int h, int gf) {               // request fragment gf of slice h
      const int j = gf & 7;
      // A swizzled address is formed where its first fragment is requested and serves every fragment that differs from it by
      // an immediate: the Q rows' kr ^ (32 j) serve the dO rows (+ TILEB), dO^T's tr ^ .. serve its second k-step and Q^T.  They are
      // opaque (hipcc neither re-forms them nor hoists them out of the slice, where they would be live across the whole tile):
      // krx lives from the S chain into the dP chain, where pks is dead; trx from the end of the dP chain on, where sc dies.
      if (gf < 16) {
        if (gf == 0) asm volatile("" : "+v"(kr));
        if (gf < 8 && j) { krx[j] = kr ^ (32 * j); asm volatile("" : "+v"(krx[j])); }
        fr[h][gf] = *(USP_LDS const u32x4*)(smem + (j ? krx[j] : kr) + (gf < 8 ? 0 : TILEB) + h * 32 * ROWB);
      } else {
        if (gf == 16) asm volatile("" : "+v"(tr));
        const int k2 = j / NDJ, dj = j % NDJ;
        if (gf < 16 + NDJ) {
          if (dj) { trx[dj] = tr ^ (64 * dj); asm volatile("" : "+v"(trx[dj])); }
          trx[4 + dj] = tr ^ (64 * dj + 32); asm volatile("" : "+v"(trx[4 + dj]));
        }
        USP_LDS const char* xb = smem + (gf < 24 ? TILEB : 0) + (2 * h + k2) * 16 * ROWB;
        const u32x2 a0 = lds_read_tr16(xb + (dj ? trx[dj] : tr));
        const u32x2 a1 = lds_read_tr16(xb + trx[4 + dj] + 2048);
        fr[h][gf] = u32x4{a0[0], a0[1], a1[0], a1[1]};
      }
    };
    // a chain STARTS from its rows' constants, the same for both key blocks: they are read ONCE, straight into key block 1's
    // accumulator, and key block 0's first MFMA takes them from there as SrcC (D = its own accumulator, chain_from) one slot in front
    // of key block 1's own first MFMA -- no registers of their own, no second read, no copy (a VALU write in front of an MFMA's SrcC
    // costs wait states).  which 0: -lse / scale -> S, 1: -delta -> dP; register r of a C tile is row (r & 3) + 8 (r >> 2) + 4 hi
    auto rd_stats = [&](int h, int which, int j) {
      const f32x4 t = *(USP_LDS const f32x4*)(stat + 4 * kTile * which + 128 * h + 32 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) (which ? dp : sc)[1][4 * j + e] = t[e];
    };
    // element n of a slice, in the order the gradient k-steps need them: n = 16 k2 + 8 kb + r8 -> [kb][8 k2 + r8]
    auto p_elem = [&](int n) {
      const int k2 = n >> 4, kb = (n >> 3) & 1, r = 8 * k2 + (n & 7);
      sc[kb][r] = fast_exp2(sc[kb][r] * c2);     // the chain computed q . k - lse / scale (-inf where masked: c2 > 0)
    };
    auto p_pack = [&](int n) {
      const int k2 = n >> 4, kb = (n >> 3) & 1, r = 8 * k2 + (n & 7);
      if (r & 1) pkp[kb][k2][(r & 7) >> 1] = E::pack2(sc[kb][r - 1], sc[kb][r]);
    };
    auto s_elem = [&](int n) {                   // dS = (the 16-bit P that feeds dV) x (dP - delta)
      const int k2 = n >> 4, kb = (n >> 3) & 1, r = 8 * k2 + (n & 7);
      const uint32_t wd = pkp[kb][k2][(r & 7) >> 1];
      dp[kb][r] = ((r & 1) ? E::hi(wd) : E::lo(wd)) * dp[kb][r];
      if (r & 1) pks[kb][k2][(r & 7) >> 1] = E::pack2(dp[kb][r - 1], dp[kb][r]);
    };
    constexpr int LAG = 2;                       // packs trail the exponentials (trans -> VALU wait state, usp_flash_bwd64.hip)
    auto elem_slot = [&](int sl) {
      if (sl >= PE0 && sl < PE1) {
#pragma unroll
        for (int n = (sl - PE0) * 32 / (PE1 - PE0); n < (sl - PE0 + 1) * 32 / (PE1 - PE0); ++n) {
          p_elem(n);
          if (n >= LAG) p_pack(n - LAG);
        }
        if (sl == PE1 - 1) {
#pragma unroll
          for (int n = 32 - LAG; n < 32; ++n) p_pack(n);
        }
      }
      if (sl >= SE0 && sl < SE1) {
#pragma unroll
        for (int n = (sl - SE0) * 32 / (SE1 - SE0); n < (sl - SE0 + 1) * 32 / (SE1 - SE0); ++n) s_elem(n);
      }
    };
    auto apply_mask = [&](int h) {               // query row i sees key j iff j <= i + off
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const int d = ow + 32 * kb + l31 - off - s0 - 4 * hi - 32 * h;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (d > (r & 3) + 8 * (r >> 2)) sc[kb][r] = USP_NEG_INF;
      }
    };
    // the first slice's first fragments and constants: one burst behind the barrier that published the tile
#pragma unroll
    for (int gf = 0; gf < LA; ++gf) rd(0, gf);
#pragma unroll
    for (int n = 0; n < 4; ++n) rd_stats(0, 0, n);
    __builtin_amdgcn_sched_barrier(0);
    static_for<2>([&](auto h_c) __attribute__((always_inline)) {
      constexpr int h = decltype(h_c)::value;
      static_for<64>([&](auto sl_c) __attribute__((always_inline)) {
        constexpr int sl = decltype(sl_c)::value;
        constexpr int gf = sl >> 1, kb = sl & 1, j = gf & 7;
        if (gf < 8) {
          if (sl == 0) U::template chain_from<MASK>(sc[0], fr[h][gf], kf[0][0], sc[1]);
          else U::template chain<MASK>(sc[kb], fr[h][gf], kf[kb][j]);
        } else if (gf < 16) {
          if (sl == 16) U::template chain_from<MASK>(dp[0], fr[h][gf], vf[0][0], dp[1]);
          else U::template chain<MASK>(dp[kb], fr[h][gf], vf[kb][j]);
        } else if (gf < 24) {
          U::template grad<MASK>(4 * kb + j % NDJ, fr[h][gf], pkp[kb][j / NDJ]);
        } else {
          U::template grad<MASK>(8 + 4 * kb + j % NDJ, fr[h][gf], pks[kb][j / NDJ]);
        }
        if (h == 0 && sl == 0) {                 // behind the first MFMA: its scalar work must not idle the matrix pipe
          __builtin_amdgcn_sched_barrier(0);
          dma_open(boff_n);
        }
        if (kb == 0) {                           // the fragment LA ahead
          if (gf + LA < 32) rd(h, gf + LA);
          else if (h == 0) rd(1, gf + LA - 32);
        }
        // the next chain's constants: -delta behind the S chain's first MFMAs, the next slice's -lse / scale late in dK
        if (sl >= 6 && sl < 10) rd_stats(h, 1, sl - 6);
        if (h == 0 && sl >= 54 && sl < 58) rd_stats(1, 0, sl - 54);
        if (h == 0 && sl >= 1 && sl <= 8) dma_piece(sl - 1);      // the next tile's pieces
        elem_slot(sl);
        __builtin_amdgcn_sched_barrier(0);
        if (MASK && sl == 15) {
          mfma_settle(sc);
          apply_mask(h);
          __builtin_amdgcn_sched_barrier(0);
        }
      });
    });
    boff_a = boff_n;
    ++tile_cur;
    USP_TM(const uint64_t tm0 = __builtin_amdgcn_s_memtime();)
    dma_drain();            // this wave's DMA pieces of the staged tile have landed
    USP_TM(const uint64_t tm1 = __builtin_amdgcn_s_memtime();)
    stats_store(boff_n);
    __syncthreads();
    USP_TM(const uint64_t tm2 = __builtin_amdgcn_s_memtime();
           tm_body += tm0 - tm_last; tm_drain += tm1 - tm0; tm_bar += tm2 - tm1; tm_last = tm2;)
  };
  const std::integral_constant<bool, false> plain;
  const std::integral_constant<bool, true> masked;
  // a head's first tile: cursors, descriptors, all of the tile's pieces, the barrier that publishes it (every wave is past the
  // barrier that ended the head in front: nobody reads a buffer any more)
  auto open_head = [&](int h) {
    pf_head(h);
    stats_fetch();
    dma_open(0);
#pragma unroll
    for (int n = 0; n < 8; ++n) dma_piece(n);
    dma_drain();
    stats_store(0);
    __syncthreads();
    tile_cur = t_begin; boff_a = 0;
  };
  for (int hh = 0; hh < gsub; ++hh) {              // head by head: the diagonal tiles first, then the plain ones
    open_head(h0 + hh);
    int it = 0;
    __builtin_amdgcn_s_waitcnt(0x0f70);
    for (; it < n_mask; ++it) step(masked);
    __builtin_amdgcn_s_waitcnt(0x0f70);
    for (; it < n_iter; ++it) step(plain);
  }

  // ---- epilogue -----------------------------------------------------------------------------------------------------------
  acc_settle();
  asm volatile("" : "+s"(p));
#pragma unroll
  for (int ten = 0; ten < 2; ++ten) {            // 0: dV, 1: dK -- the wave stores both tensors' rows of its keys
    // 16-bit final output of this tensor, rows 16-byte aligned, nothing accumulated, no head-split partials
    const bool wide = !p->split && (p->wide16 & (ten == 0 ? 4 : 2)) != 0;
    const float mul = ten == 0 ? 1.f : p->scale;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int orow = ow + 32 * kb + l31;
      f32x16 acc[NDJ];
#pragma unroll
      for (int dj = 0; dj < NDJ; ++dj) acc_read(8 * ten + 4 * kb + dj, acc[dj]);
      if (wide) {
        const int orow_c = orow < p->Sk ? orow : 0;
        char* row16 = ten == 0 ? p->dv16 + 2 * (b * p->dv16_sb + (int64_t)orow_c * p->dv16_ss + hkv * p->dv16_sh)
                               : p->dk16 + 2 * (b * p->dk16_sb + (int64_t)orow_c * p->dk16_ss + hkv * p->dk16_sh);
        store_row16_wide<E, NDJ>(row16, acc, mul, hi, orow < p->Sk);
      } else if (orow < p->Sk) {
        float* o32;
        char* o16 = nullptr;
        int accf;
        if (p->split) {                            // partial slab of (head run, cut)
          const int64_t wo = (((int64_t)(g * p->qsplit + cut) * p->ws_rows + (int64_t)b * p->Sk + orow) * p->Hkv + hkv) * D;
          o32 = (ten == 0 ? p->ws_dv : p->ws_dk) + wo; accf = 0;
        } else if (ten == 0) {
          o32 = p->dv + b * p->dv_sb + (int64_t)orow * p->dv_ss + hkv * p->dv_sh; accf = p->accum_dv;
          if (p->dv16) o16 = p->dv16 + 2 * (b * p->dv16_sb + (int64_t)orow * p->dv16_ss + hkv * p->dv16_sh);
        } else {
          o32 = p->dk + b * p->dk_sb + (int64_t)orow * p->dk_ss + hkv * p->dk_sh; accf = p->accum_dk;
          if (p->dk16) o16 = p->dk16 + 2 * (b * p->dk16_sb + (int64_t)orow * p->dk16_ss + hkv * p->dk16_sh);
        }
        store_row32_acc<E, NDJ>(o32, o16, acc, mul, hi, accf);
      }
    }
  }
// (dev build: behind the stores -- a device printf in front of them may use the accumulator registers)
USP_TM(
  if (pass == 0 && lane == 0 && (blockIdx.x % 61) == 0)
    printf("TM wg %3d wave %d blk %2d n_iter %3d n_mask %d : body %8llu drain %7llu barrier %7llu  (per tile %5llu / %4llu / %4llu)\n",
           (int)blockIdx.x, wave, blk, n_iter, n_mask, (unsigned long long)tm_body, (unsigned long long)tm_drain,
           (unsigned long long)tm_bar, (unsigned long long)(tm_body / (n_iter * gsub + 1)), (unsigned long long)(tm_drain / (n_iter * gsub + 1)),
           (unsigned long long)(tm_bar / (n_iter * gsub + 1)));
)
  }  // next item
}

bool dkdv64u_serves(const BwdParams& p_in) { return dkdv64_serves(p_in); }

bool launch_dkdv64u(const BwdParams& p_in, int dtype, bool causal, hipStream_t st, int* rc) {
  if (!dkdv64u_serves(p_in)) return false;
  BwdParams p = p_in;
  p.wide16 = ((p.dk16 && !p.accum_dk && tensor_aligned(p.dk16, p.dk16_sb, p.dk16_ss, p.dk16_sh, 16, 8)) ? 2 : 0) |
             ((p.dv16 && !p.accum_dv && tensor_aligned(p.dv16, p.dv16_sb, p.dv16_ss, p.dv16_sh, 16, 8)) ? 4 : 0);
  p.nblk = (p.Sk + 255) / 256;
  p.n_items = p.B * p.Hkv * p.nblk * p.ngrp * p.qsplit;
  const int grid = persistent_grid(p.n_items, device_cus(), p.interleave);      // persistent: one workgroup per CU
  constexpr size_t lds = 3 * (2 * kTile * 128 * 2 + 2 * kTile * 4);
  with_dtype_causal(dtype, causal, [&](auto dt, auto c) {
    hipLaunchKernelGGL((flash_bwd_dkdv64u_kernel<decltype(dt)::value, decltype(c)::value>), dim3(grid), dim3(256), lds, st, p);
  });
  *rc = launched();
  return true;
}

}  // namespace usp
