// The top-p cut over weights that are GIVEN (C ABI: usp_block_select_weights; include/usp_hip.h): the selector behind
// usp_block_antidiag_weights, and an exact selector behind the usp_block_attn_mass of an earlier call.  A translation unit of its
// own beside usp_block_select_top_p.hip; the search itself is that kernel's, shared as text (usp_block_top_p_cut.inc: the
// contract of what an includer must have in scope stands there and at each include site).  No atomics, nothing read on the host, no inline assembly.
#include "usp_host.hpp"

namespace usp {

// (the include declares kTopPThreads, weight_key, wave_sum, wave_max, block_sum, block_max at namespace scope)
#define USP_TOP_P_HELPERS
#include "usp_block_top_p_cut.inc"
#undef USP_TOP_P_HELPERS

// The same cut over weights that are GIVEN (C ABI: usp_block_select_weights): one workgroup per (b, h, I) reads the row
// w[b][h][I][0 .. nbk) as it stands into LDS -- thread t its blocks J = t, t + 256, ..., the blocks it alone reads again -- and
// runs the cut (usp_block_top_p_cut.inc).  The producers: usp_block_antidiag_weights, or the usp_block_attn_mass of an earlier call.
struct BlockSelectWeightsArgs {
  const float* w;
  int64_t w_sb, w_sh, w_sr;    // element strides of batch, head, row block
  unsigned char* mask;
  int64_t sb, sh, sr;          // byte strides of batch, head, row block
  int Hq, nbq, nbk, row_block0;
  float top_p;
  int causal, keep_first, keep_local;
};

__global__ __launch_bounds__(kTopPThreads) void block_select_weights_kernel(const BlockSelectWeightsArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t top_p_lds[];   // [nbk weights, padded to 4][2 x 4 wave slots]
  float* const wts = (float*)top_p_lds;
  float* const slots = wts + ((a.nbk + 3) & ~3);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t id = blockIdx.x;                   // (b, h, I), I fastest
  const int I = (int)(id % a.nbq);
  const int64_t bh = id / a.nbq;
  const int h0 = (int)(bh % a.Hq), b = (int)(bh / a.Hq), nh = 1;
  const int Ig = a.row_block0 + I;
  const int nbk = a.nbk;
  // (the include reads Ig, nbk, a.causal, a.keep_first, a.keep_local and declares nv, kf, lo, hi, search, phase)
#define USP_TOP_P_ROW
#include "usp_block_top_p_cut.inc"
#undef USP_TOP_P_ROW
  if (search) {
    const float* const w = a.w + b * a.w_sb + h0 * a.w_sh + I * a.w_sr;
    for (int J = t; J < nbk; J += kTopPThreads) wts[J] = w[J];
  }
  // (the include reads those and t, lane, wave, slots, wts, a.top_p, a.mask, a.sb, a.sh, a.sr, b, h0, nh, I; it writes the mask row(s))
#define USP_TOP_P_CUT
#include "usp_block_top_p_cut.inc"
#undef USP_TOP_P_CUT
}

}  // namespace usp

extern "C" int usp_block_select_weights(const float* w, int64_t w_stride_b, int64_t w_stride_h, int64_t w_stride_row, int32_t B,
                                        int32_t Hq, int32_t nbq, int32_t nbk, int32_t row_block0, int32_t causal, float top_p,
                                        int32_t keep_first, int32_t keep_local, void* mask, int64_t mask_stride_b,
                                        int64_t mask_stride_h, int64_t mask_stride_row, void* stream) {
  using namespace usp;
  launch_kinds_reset();
  if (!w || !mask || B <= 0 || Hq <= 0 || nbq <= 0 || nbk <= 0) return USP_EINVAL;
  if (row_block0 < 0 || keep_first < 0 || keep_local < 0 || (causal && keep_local < 1)) return USP_EINVAL;
  if (!(top_p > 0.f) || !(top_p <= 1.f)) return USP_EINVAL;          // NaN, <= 0, > 1
  if (w_stride_b < 0 || w_stride_h < 0 || w_stride_row < 0) return USP_EINVAL;
  if (mask_stride_b < 0 || mask_stride_h < 0 || mask_stride_row < 0) return USP_EINVAL;
  if (nbk > USP_BLOCK_SELECT_MAX_BLOCKS || (int64_t)row_block0 + nbq > (1 << 30)) return USP_EUNSUPPORTED;
  if (!aligned(w, 4)) return USP_EUNSUPPORTED;
  const int64_t grid = (int64_t)B * Hq * nbq;
  if (grid >= (1LL << 31)) return USP_EUNSUPPORTED;
  BlockSelectWeightsArgs a;
  a.w = w; a.w_sb = w_stride_b; a.w_sh = w_stride_h; a.w_sr = w_stride_row;
  a.mask = (unsigned char*)mask; a.sb = mask_stride_b; a.sh = mask_stride_h; a.sr = mask_stride_row;
  a.Hq = Hq; a.nbq = nbq; a.nbk = nbk; a.row_block0 = row_block0;
  a.top_p = top_p; a.causal = causal ? 1 : 0; a.keep_first = keep_first; a.keep_local = keep_local;
  const size_t lds = ((size_t)((nbk + 3) & ~3) + 8) * 4;             // <= 32 KiB + 32 bytes
  hipLaunchKernelGGL(block_select_weights_kernel, dim3((unsigned)grid), dim3(kTopPThreads), lds, (hipStream_t)stream, a);
  launch_kinds_note(USP_KIND_BLOCK_SELECT_WEIGHTS);
  return launched();
}
