// List builder of the block-sparse attention launches (C ABI: usp_block_list_bytes, usp_flash_fwd_bsp, usp_flash_bwd_bsp;
// include/usp_hip.h).  HBM-bound helper: turns the 128 x 128 block mask (one byte per block, three strides, last dimension dense)
// into compact int32 lists in the caller's workspace (layout: usp_host.hpp, BlockLists), at the kernels' tile granularity:
//   family F, per (b, h, row block r):            [count, ascending 64-key tiles of the live key blocks]            (forward)
//   family Q, per (b, h, pair of row blocks i):   [count, ascending 4 * tile + (bit 0: live for 2i, bit 1: for 2i + 1)]  (dQ)
//   family T, per (b, h, key block c):            [count, ascending 64-row tiles of the live row blocks]            (dK/dV)
// Under `causal` the blocks above the diagonal are dropped, so the kernels never stream them.  The second tile of the last block
// is dropped where the sequence ends in front of it.  One wave per list: 64 blocks per step, compacted with ballot and popcount;
// no atomics, every list is written by one wave in a fixed order.
#include "usp_host.hpp"

namespace usp {

struct BlockListArgs {
  const unsigned char* mask;
  int64_t sb, sh, sr;          // byte strides of batch, head, row block
  int* ws;
  BlockLists l;
  int ntq, ntk;                // 64-row / 64-key tiles of the launch
  int causal, which;           // which: bit 0 = F, bit 1 = Q, bit 2 = T
};

__global__ __launch_bounds__(256) void block_lists_kernel(const BlockListArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);     // one wave per list
  const int64_t nF = a.l.bh * a.l.nrb, nQ = a.l.bh * a.l.nqb, nT = a.l.bh * a.l.nkb;
  if (id >= nF + nQ + nT) return;
  const int fam = id < nF ? 0 : (id < nF + nQ ? 1 : 2);
  if (!((a.which >> fam) & 1)) return;
  const int64_t loc = fam == 0 ? id : (fam == 1 ? id - nF : id - nF - nQ);
  const int per = fam == 0 ? a.l.nrb : (fam == 1 ? a.l.nqb : a.l.nkb);
  const int blk = (int)(loc % per);
  const int64_t bh = loc / per;
  const int h = (int)(bh % a.l.hq), b = (int)(bh / a.l.hq);
  const unsigned char* const m = a.mask + b * a.sb + h * a.sh;
  int* const out = a.ws + (fam == 0 ? loc * a.l.lf : (fam == 1 ? a.l.off_q + loc * a.l.lf : a.l.off_t + loc * a.l.lt));
  const int n_in = fam == 2 ? a.l.nrb : a.l.nkb;       // blocks along the listed side
  const int n_tiles = fam == 2 ? a.ntq : a.ntk;        // ... and its 64-wide tiles
  int count = 0;
  for (int c0 = 0; c0 < n_in; c0 += 64) {
    const int c = c0 + lane;
    int bits = 0;
    if (c < n_in) {
      if (fam == 0) {
        bits = (m[(int64_t)blk * a.sr + c] != 0 && (!a.causal || c <= blk)) ? 1 : 0;
      } else if (fam == 1) {
        const int r0 = 2 * blk, r1 = 2 * blk + 1;
        if (m[(int64_t)r0 * a.sr + c] != 0 && (!a.causal || c <= r0)) bits |= 1;
        if (r1 < a.l.nrb && m[(int64_t)r1 * a.sr + c] != 0 && (!a.causal || c <= r1)) bits |= 2;
      } else {
        bits = (m[(int64_t)c * a.sr + blk] != 0 && (!a.causal || blk <= c)) ? 1 : 0;
      }
    }
    const bool live = bits != 0;
    const unsigned long long bal = __ballot(live);
    const int pos = count + 2 * __builtin_popcountll(bal & ((1ull << lane) - 1ull));
    const bool second = 2 * c + 1 < n_tiles;           // (false for the last block alone: it is the last entry)
    if (live) {
      out[1 + pos] = fam == 1 ? 4 * (2 * c) + bits : 2 * c;
      if (second) out[1 + pos + 1] = fam == 1 ? 4 * (2 * c + 1) + bits : 2 * c + 1;
    }
    count += 2 * __builtin_popcountll(bal) - __builtin_popcountll(__ballot(live && !second));
  }
  if (lane == 0) out[0] = count;
}

int launch_block_lists(const void* mask, int64_t sb, int64_t sh, int64_t sr, int* ws, const BlockLists& l, int Sq, int Sk, bool causal,
                       int which, hipStream_t st) {
  BlockListArgs a;
  a.mask = (const unsigned char*)mask; a.sb = sb; a.sh = sh; a.sr = sr;
  a.ws = ws; a.l = l;
  a.ntq = (Sq + 63) / 64; a.ntk = (Sk + 63) / 64;
  a.causal = causal ? 1 : 0; a.which = which;
  const int64_t lists = l.bh * ((int64_t)l.nrb + l.nqb + l.nkb);
  hipLaunchKernelGGL(block_lists_kernel, dim3((unsigned)((lists + 3) / 4)), dim3(256), 0, st, a);
  return launched();
}

}  // namespace usp

// The builder alone: the lists of `which` (1 forward, 2 dQ, 4 dK/dV; any sum) as usp_flash_fwd_bsp / usp_flash_bwd_bsp build them
extern "C" int usp_block_lists_build(const void* mask, int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_row, int32_t B,
                                     int32_t Hq, int32_t S, int32_t causal, int32_t which, void* lists, void* stream) {
  using namespace usp;
  if (!mask || !lists || !aligned(lists, 4) || B <= 0 || Hq <= 0 || S <= 0 || mask_stride_b < 0 || mask_stride_h < 0 ||
      mask_stride_row < 0 || (which & ~7) || !which)
    return USP_EINVAL;
  const int nb = (S + 127) / 128;
  return launch_block_lists(mask, mask_stride_b, mask_stride_h, mask_stride_row, (int*)lists, block_lists(B, Hq, nb, nb), S, S, causal != 0,
                            which, (hipStream_t)stream);
}

extern "C" int64_t usp_block_list_bytes(int32_t B, int32_t Hq, int32_t n_row_blocks, int32_t n_key_blocks) {
  if (B <= 0 || Hq <= 0 || n_row_blocks <= 0 || n_key_blocks <= 0) return 0;
  return usp::block_lists(B, Hq, n_row_blocks, n_key_blocks).ints * 4;
}
