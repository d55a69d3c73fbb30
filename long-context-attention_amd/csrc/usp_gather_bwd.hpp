// The gathered-key backward (usp_flash_bwd_gather.hip): the argument block of its three kernels.  The tile image and the lane maps
// are the forward's (usp_gather.hpp), untouched.
#pragma once
#include "usp_gather.hpp"

namespace usp {

// One gradient tensor as the kernels finish it:  value = (add ? f32[...] : 0) + this launch's share, written to h16 (rounded once)
// when h16 is set, to f32 otherwise.  f32 is the caller's fp32 tensor or the band's fp32 result in the workspace; NULL only when
// nothing is added and h16 is set.
struct GatherGrad {
  float* f32; int64_t f_sb, f_ss, f_sh;
  char* h16; int64_t h_sb, h_ss, h_sh;
  int add;
};

struct BwdArgsGather {
  const char* dout; const char* q; const char* k; const char* v;
  const float* lse; const float* delta;
  int64_t do_sb, do_ss, do_sh, q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss, v_sh;
  int64_t lse_sb, lse_sh, dl_sb, dl_sh;
  GatherGrad gq, gk, gv;
  float* dk_list; float* dv_list;       // fp32 partials (B, Hq, n_pad, D): row (b, h, pos) belongs to entry pos of the list of (b, h)
  int n_pad;                            // n_idx rounded up to whole 64-entry tiles
  const int* kidx;                      // as FwdArgsGather
  int64_t kidx_sb, kidx_sh;
  int n_idx;
  int B, Sq, Sk, Hq, Hkv, G, D;
  int nq, n_items;                      // dQ launch: 128-row tiles, items (set in launch_bwd_gather)
  int causal_off;
  float scale, scale_log2;
  int win_on, left;                     // the band the LISTED part leaves out: row i takes entry e iff e < d_i - left (no window: e <= d_i)
  int k_bytes, v_bytes, q_bytes, do_bytes;   // extent of one (batch, head) plane from its first row, in bytes (< 2^31)
  int interleave, walk_g;
};
// which: bit 0 = the dQ launch, bit 1 = the dK/dV launch and the scatter behind it
int launch_bwd_gather(const BwdArgsGather& p, int D, int dtype, int which, hipStream_t st);

}  // namespace usp
