// Blockwise flash-attention backward for gfx950.  C ABI: usp_flash_bwd (include/usp_hip.h).
// Replaces the reference's `bwd-only` block kernel (yunchang/kernels/attention.py:205-250) plus the
// fp32 accumulation the ring schedules do on its results (zigzag_ring_flash_attn.py:147-170).
//
// Two launches, no atomics, deterministic:
//   dQ     (flash_bwd_kernel)      : workgroup = 8 waves x 32 query rows; streams K,V tiles (64 keys) through LDS.
//                                    lane owns a query row:  S^T = K Q^T, dP^T = V dO^T, dQ^T += K^T dS^T
//   dK, dV (flash_bwd_dkdv_kernel) : workgroup = 8 waves, 128 keys, two roles (below); the one-wave-per-SIMD form of it
//                                    lives in usp_flash_bwd64.hip and serves the dense D = 128 launches.
// Each is a body of its own (usp_flash_bwd_dq_body.inc, usp_flash_bwd_dkdv_body.inc).  What they share is the layout: the
// streamed pair of tiles -- K and V for dQ, Q and dO for dK/dV -- lies in LDS row-major with a 16-byte-slot XOR swizzle chosen
// so that BOTH ds_read_b128 row reads and ds_read_b64_tr_b16 column reads are bank-conflict free; the wave's own rows (Q and dO
// fragments for dQ; K or V fragments, by role, for dK/dV) stay in registers as B operands; the chains S = K Q^T, dP = V dO^T
// (dQ) and S = Q K^T, dP = dO V^T (dK/dV) read the tiles by rows, the gradient MFMAs read them transposed.  As in the forward,
// no cross-lane shuffle is needed for P / dS: the k-step order of the gradient MFMAs is defined as the order the S accumulator
// holds rows.  Which tiles an item streams and which of them are live or masked: usp_tile_range.h.
#include "usp_bwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

// Every kernel of the two launches is a shared body under a __global__ template that gives it a name, an argument block `p_in`
// and CAUSAL; the body derives its switches from the block's type ("How a kernel variant is declared").  The variants
// live in usp_flash_bwd_{alibi,dropout,doc,span,bsp}.hip.
// SC (BwdArgsSC), logit soft-capping (USP_ATTN_SOFTCAP): with t = tanh(S/cap) of the raw (masked) score,
// P = exp2(cap*log2e*t - lse2) (0 where masked) and dS = P (dP - delta) (1 - t^2), in place; the epilogue's `scale` is
// unchanged.
template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_kernel(const BwdParams p_in) {
#include "usp_flash_bwd_dq_body.inc"
}

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_softcap_kernel(const BwdArgsSC p_in) {
#include "usp_flash_bwd_dq_body.inc"
}

// ======================================================================================================
// dK/dV, role-specialised waves.
//
// A single-role wave needs K AND V fragments (64 regs) plus dK AND dV accumulators (128 regs) per wave: > 256
// registers, i.e. ONE wave per SIMD, and a lone wave can hide only ~5 instructions per MFMA (measured:
// 57 % of its cycles are active issue, MFMA pipe 32 % busy).  Here every 32-key slice is served by TWO
// waves that sit on the same SIMD (wave w and w + 4):
//   role A (waves 0-3): S = Q K^T -> P = exp2(S*c - lse)  -> dV^T += dO^T P      (K frags, dV acc)
//   role B (waves 4-7): dP = dO V^T, P from A, dS = P*(dP - delta) -> dK^T += Q^T dS (V frags, dK acc)
// A hands P (bf16, 4 KiB per 64x32 block, raw register image: lane-linear ds_write/ds_read_b128) to B
// through LDS; B runs ONE TILE BEHIND A, so the hand-off is ordered by the per-tile s_barrier that
// exists anyway (double-buffered P slots, triple-buffered Q/dO tiles).  No recompute: 32 MFMAs per
// wave and tile instead of 64, < 256 registers per wave, two waves per SIMD with complementary
// MFMA / transcendental mixes.
// SC (logit soft-capping, PA = BwdArgsSC): role A computes t = tanh(S/cap) and P = exp2(cap*log2e*t - lse2) (0 where
// masked), uses P for its own dV MFMAs and hands P (1 - t^2) to B instead of P: B's dS = P_in (dP - delta) is then the
// capped dS with no change to role B and no extra LDS.
// ======================================================================================================

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_dkdv_kernel(const BwdParams p_in) {
#include "usp_flash_bwd_dkdv_body.inc"
}

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_dkdv_softcap_kernel(const BwdArgsSC p_in) {
#include "usp_flash_bwd_dkdv_body.inc"
}

// dst[b,s,h,:] (+)= sum_g ws[g][row][h][:]   -- combines the per-query-head dK / dV partials.
// Dense: row = b*S + s.  Packed: (b, s) runs over B x max rows; sequence b owns rows first_b + s, s < rows_b.
template <int D, int DT>
__global__ __launch_bounds__(256) void reduce_heads_kernel(const BwdParams p) {
  using E = Elem<DT>;
  constexpr int C4 = D / 4;
  const int S = p.Sk, H = p.Hkv;
  const int64_t total = (int64_t)p.B * S * H * C4;
  const int64_t gstride = p.ws_rows * H * D;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c4 = (int)(i % C4);
    const int64_t r = i / C4;
    const int h = (int)(r % H);
    const int64_t bs = r / H;
    const int sidx = (int)(bs % S);
    const int b = (int)(bs / S);
    int64_t row = sidx, wrow = bs, bb = b;       // row inside dk/dv (with b), row inside a workspace slab
    if (p.seq_k != nullptr) {
      if (sidx >= p.seq_k[2 * b + 1] || p.seq_q[2 * b + 1] <= 0) continue;
      row = wrow = p.seq_k[2 * b] + sidx;
      bb = 0;
    }
    const int64_t e = 4 * c4;
    float* pk = p.dk ? p.dk + bb * p.dk_sb + row * p.dk_ss + h * p.dk_sh + e : nullptr;
    float* pv = p.dv ? p.dv + bb * p.dv_sb + row * p.dv_ss + h * p.dv_sh + e : nullptr;
    f32x4 ak = p.accum_dk ? *(const f32x4*)pk : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 av = p.accum_dv ? *(const f32x4*)pv : f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t o = (wrow * H + h) * D + e;
    for (int g = 0; g < p.nslab; ++g) {
      ak += *(const f32x4*)(p.ws_dk + g * gstride + o);
      av += *(const f32x4*)(p.ws_dv + g * gstride + o);
    }
    if (p.dk16) {
      char* hk = p.dk16 + 2 * (bb * p.dk16_sb + row * p.dk16_ss + h * p.dk16_sh + e);
      *(u32x2*)hk = u32x2{E::pack2(ak[0], ak[1]), E::pack2(ak[2], ak[3])};
    } else {
      *(f32x4*)pk = ak;
    }
    if (p.dv16) {
      char* hv = p.dv16 + 2 * (bb * p.dv16_sb + row * p.dv16_ss + h * p.dv16_sh + e);
      *(u32x2*)hv = u32x2{E::pack2(av[0], av[1]), E::pack2(av[2], av[3])};
    } else {
      *(f32x4*)pv = av;
    }
  }
}

// dq[b,s,h,:] (+)= sum_cut ws_dq[cut][b][s][h][:]   -- combines the dQ partials of a key-cut launch (dense only).
template <int D, int DT>
__global__ __launch_bounds__(256) void reduce_cuts_kernel(const BwdParams p) {
  using E = Elem<DT>;
  constexpr int C4 = D / 4;
  const int64_t total = (int64_t)p.B * p.Sq * p.Hq * C4;
  const int64_t cstride = (int64_t)p.B * p.Sq * p.Hq * D;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c4 = (int)(i % C4);
    int64_t r = i / C4;
    const int h = (int)(r % p.Hq); r /= p.Hq;
    const int sidx = (int)(r % p.Sq);
    const int b = (int)(r / p.Sq);
    const int64_t e = 4 * c4;
    float* pq = p.dq ? p.dq + b * p.dq_sb + (int64_t)sidx * p.dq_ss + h * p.dq_sh + e : nullptr;
    f32x4 a = p.accum_dq ? *(const f32x4*)pq : f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t o = (((int64_t)b * p.Sq + sidx) * p.Hq + h) * D + e;
    for (int c = 0; c < p.ksplit; ++c) a += *(const f32x4*)(p.ws_dq + c * cstride + o);
    if (p.dq16) {
      char* hq = p.dq16 + 2 * (b * p.dq16_sb + (int64_t)sidx * p.dq16_ss + h * p.dq16_sh + e);
      *(u32x2*)hq = u32x2{E::pack2(a[0], a[1]), E::pack2(a[2], a[3])};
    } else {
      *(f32x4*)pq = a;
    }
  }
}

static int reduce_grid(int64_t items) { return (int)((items + 255) / 256 > 2048 ? 2048 : (items + 255) / 256); }

// What usp_flash_bwd_alibi / _dropout / _doc add to a plain call; nothing set: usp_flash_bwd.  The entry points fill the slopes and
// their stride, dc and doc as given; flash_bwd_call checks them and fills al.al_diag and dr, the kernels' dropout block (dr.t == 0:
// off).
struct BwdExtras {
  BwdAlibi al{};
  DropoutCall dc{};
  BwdDoc doc{};
  BwdSpan span{};
  BspCall bsp{};                 // (usp_flash_bwd_bsp: the block mask and the workspace of its lists)
  Dropout dr{};
  bool any() const { return al.al_slopes || dr.t || doc.row_lo || doc.key_hi || span.row_hi || span.key_lo || bsp.mask; }
};

// dK/dV of a call: the one-wave-per-SIMD kernel (4 waves x 64 keys, usp_flash_bwd64.hip) where `row64` allows it and it serves
// the launch, the 8-wave kernel otherwise; then the sum over the partial slabs of a head-split / cut launch.
template <int D, int DT>
static int launch_dkdv(BwdArgsSC& p, const BwdExtras& x, bool causal, hipStream_t st, bool row64, int keys) {
  p.nblk = (p.Sk + 127) / 128;
  p.n_items = p.B * p.Hkv * p.nblk * p.ngrp * p.qsplit;
  int rc = USP_ELAUNCH;
  if (row64 && keys == 256 && launch_dkdv64u(p, DT, causal, st, &rc)) {      // 256-key items (usp_flash_bwd64u.hip; dkdv_keys_of)
    if (rc != USP_OK) return rc;
    launch_kinds_note(USP_KIND_DKDV_ROW64 | USP_KIND_DKDV_KEYS256);
  } else if (row64 && launch_dkdv64(p, DT, causal, st, &rc)) {
    if (rc != USP_OK) return rc;
    launch_kinds_note(USP_KIND_DKDV_ROW64);
  } else {
    // the 8-wave dK/dV kernel addresses the Q / dO tiles of a head by a 32-bit byte offset from the head's first row
    if ((int64_t)p.Sq * p.q_ss * 2 >= (1LL << 31) || (int64_t)p.Sq * p.do_ss * 2 >= (1LL << 31)) return USP_EUNSUPPORTED;
    // persistent: one workgroup per CU (the kernel fits once per CU)
    const int grid = persistent_grid(p.n_items, device_cus(), p.interleave);
    constexpr size_t lds = 3 * (2 * kTile * D * 2 + 2 * kTile * 4) + 4 * 2 * 4096;
    p.sched_lds = (int)lds;
    const size_t lds_q = lds + (p.sched ? 16 : 0);   // + the item queue's two slots
    const BwdParams pb = p;                        // the argument block of the kernels without softcap
    if (x.al.al_slopes) {                          // ALiBi: instantiations of their own (usp_flash_bwd_alibi.hip)
      BwdArgsAL pa;
      static_cast<BwdParams&>(pa) = pb;
      static_cast<BwdAlibi&>(pa) = x.al;
      if (int rc2 = launch_dkdv_alibi(pa, D, DT, causal, grid, lds_q, st)) return rc2;
    } else if (x.dr.t) {                           // dropout: likewise (usp_flash_bwd_dropout.hip)
      BwdArgsDR pd;
      static_cast<BwdParams&>(pd) = pb;
      static_cast<Dropout&>(pd) = x.dr;
      if (int rc2 = launch_dkdv_dropout(pd, D, DT, causal, grid, lds_q, st)) return rc2;
    } else if (x.bsp.mask) {                       // block-sparse mask: likewise (usp_flash_bwd_bsp.hip); the lists are built by now
      const BlockLists& bl = x.bsp.layout;
      BwdArgsBSP pd;
      static_cast<BwdParams&>(pd) = pb;
      pd.bsp_lists = x.bsp.lists + bl.off_t; pd.bsp_stride = bl.lt;
      if (int rc2 = launch_dkdv_bsp(pd, D, DT, causal, grid, lds_q, st)) return rc2;
    } else if (x.span.key_lo) {                    // span bound: likewise (usp_flash_bwd_span.hip), never causal
      BwdArgsSPAN pd;
      static_cast<BwdParams&>(pd) = pb;
      static_cast<BwdDoc&>(pd) = x.doc;
      static_cast<BwdSpan&>(pd) = x.span;
      if (int rc2 = launch_dkdv_span(pd, D, DT, grid, lds_q, st)) return rc2;
    } else if (x.doc.key_hi) {                     // document mask: likewise (usp_flash_bwd_doc.hip)
      BwdArgsDOC pd;
      static_cast<BwdParams&>(pd) = pb;
      static_cast<BwdDoc&>(pd) = x.doc;
      if (int rc2 = launch_dkdv_doc(pd, D, DT, causal, grid, lds_q, st)) return rc2;
    } else
    with_causal(causal, [&](auto c) {
      constexpr bool C = decltype(c)::value;
      if (p.cap_on) hipLaunchKernelGGL((flash_bwd_dkdv_softcap_kernel<D, DT, C>), dim3(grid), dim3(512), lds_q, st, p);
      else hipLaunchKernelGGL((flash_bwd_dkdv_kernel<D, DT, C>), dim3(grid), dim3(512), lds_q, st, pb);
    });
    launch_kinds_note(USP_KIND_DKDV_WAVE8);
    if (launched() != USP_OK) return USP_ELAUNCH;
  }
  if (!p.split) return USP_OK;
  const BwdParams pb = p;
  hipLaunchKernelGGL((reduce_heads_kernel<D, DT>), dim3(reduce_grid((int64_t)p.B * p.Sk * p.Hkv * (D / 4))), dim3(256), 0, st, pb);
  if (launched() != USP_OK) return USP_ELAUNCH;
  launch_kinds_note(USP_KIND_REDUCE_HEADS);
  return USP_OK;
}

// dQ of a call: the one-wave-per-SIMD kernel (4 waves x 64 query rows, usp_flash_bwd_dq64.hip) or the 8-wave kernel, as above
template <int D, int DT>
static int launch_dq(BwdArgsSC& p, const BwdExtras& x, bool causal, hipStream_t st, bool row64) {
  int rc = USP_ELAUNCH;
  if (row64 && launch_dq64(p, DT, causal, st, &rc)) {
    if (rc == USP_OK) launch_kinds_note(USP_KIND_DQ_ROW64);
    return rc;
  }
  p.nblk = (p.Sq + 255) / 256;
  p.n_items = p.B * p.Hq * p.nblk * p.ksplit;
  const int grid = persistent_grid(p.n_items, device_cus(), p.interleave);
  constexpr size_t lds = 2 * (2 * kTile * D * 2);
  p.sched_lds = (int)lds;
  const size_t lds_q = lds + (p.sched ? 16 : 0);   // + the item queue's two slots
  const BwdParams pb = p;
  if (x.al.al_slopes) {                            // ALiBi: instantiations of their own (usp_flash_bwd_alibi.hip)
    BwdArgsAL pa;
    static_cast<BwdParams&>(pa) = pb;
    static_cast<BwdAlibi&>(pa) = x.al;
    if (int rc2 = launch_dq_alibi(pa, D, DT, causal, grid, lds_q, st)) return rc2;
  } else if (x.dr.t) {                             // dropout: likewise (usp_flash_bwd_dropout.hip)
    BwdArgsDR pd;
    static_cast<BwdParams&>(pd) = pb;
    static_cast<Dropout&>(pd) = x.dr;
    if (int rc2 = launch_dq_dropout(pd, D, DT, causal, grid, lds_q, st)) return rc2;
  } else if (x.bsp.mask) {                         // block-sparse mask: likewise (usp_flash_bwd_bsp.hip); the lists are built by now
    const BlockLists& bl = x.bsp.layout;
    BwdArgsBSP pd;
    static_cast<BwdParams&>(pd) = pb;
    pd.bsp_lists = x.bsp.lists + bl.off_q; pd.bsp_stride = bl.lf;
    if (int rc2 = launch_dq_bsp(pd, D, DT, causal, grid, lds_q, st)) return rc2;
  } else if (x.span.row_hi) {                      // span bound: likewise (usp_flash_bwd_span.hip), never causal
    BwdArgsSPAN pd;
    static_cast<BwdParams&>(pd) = pb;
    static_cast<BwdDoc&>(pd) = x.doc;
    static_cast<BwdSpan&>(pd) = x.span;
    if (int rc2 = launch_dq_span(pd, D, DT, grid, lds_q, st)) return rc2;
  } else if (x.doc.row_lo) {                       // document mask: likewise (usp_flash_bwd_doc.hip)
    BwdArgsDOC pd;
    static_cast<BwdParams&>(pd) = pb;
    static_cast<BwdDoc&>(pd) = x.doc;
    if (int rc2 = launch_dq_doc(pd, D, DT, causal, grid, lds_q, st)) return rc2;
  } else
  with_causal(causal, [&](auto c) {
    constexpr bool C = decltype(c)::value;
    if (p.cap_on) hipLaunchKernelGGL((flash_bwd_softcap_kernel<D, DT, C>), dim3(grid), dim3(512), lds_q, st, p);
    else hipLaunchKernelGGL((flash_bwd_kernel<D, DT, C>), dim3(grid), dim3(512), lds_q, st, pb);
  });
  if (launched() != USP_OK) return USP_ELAUNCH;
  launch_kinds_note(USP_KIND_DQ_WAVE8);
  return USP_OK;
}

// the sum over the dQ partials of a key-cut launch; same stream: the cuts' partials are complete when this starts
template <int D, int DT>
static int launch_reduce_cuts(const BwdParams& p, hipStream_t st) {
  hipLaunchKernelGGL((reduce_cuts_kernel<D, DT>), dim3(reduce_grid((int64_t)p.B * p.Sq * p.Hq * (D / 4))), dim3(256), 0, st, p);
  launch_kinds_note(USP_KIND_REDUCE_CUTS);
  return launched();
}

template <int D, int DT>
static int launch_bwd(BwdArgsSC p, const BwdExtras& x, bool causal, hipStream_t st, int force, int skip, int keys) {
  const bool want_dkdv = !(skip & USP_BWD_SKIP_DKDV), want_dq = !(skip & USP_BWD_SKIP_DQ);
  // per call, `force` = USP_FORCE_ROW64 / USP_FORCE_WAVE32 (include/usp_hip.h) picks the family; forced onto the 64-row
  // family, only the launches that will run have to be served
  if ((force & USP_FORCE_ROW64) && !(D == 128 && (!want_dkdv || dkdv64_serves(p)) && (!want_dq || dq64_serves(p))))
    return USP_EUNSUPPORTED;
  // the 64-row kernels: head dim 128; their hand-pinned pipelines have no softcap step
  const bool row64 = D == 128 && !(force & USP_FORCE_WAVE32) && !p.cap_on && !x.any();   // (... and no ALiBi, dropout or document step)
  // an item width forced on the dK/dV launch (USP_DKDV_KEYS256 / _KEYS128): that launch must be one the 64-row family serves
  if (want_dkdv && (force & (USP_DKDV_KEYS256 | USP_DKDV_KEYS128)) && !(row64 && dkdv64u_serves(p))) return USP_EUNSUPPORTED;
  int rc = USP_OK;
  if (x.bsp.mask) {                               // the lists of the launches that run, once, in front of them on the same stream
    rc = launch_block_lists(x.bsp.mask, x.bsp.sb, x.bsp.sh, x.bsp.sr, x.bsp.lists, x.bsp.layout, p.Sq, p.Sk, causal, (want_dq ? 2 : 0) | (want_dkdv ? 4 : 0), st);
    if (rc != USP_OK) return rc;
  }
  if (want_dkdv && (rc = launch_dkdv<D, DT>(p, x, causal, st, row64, keys)) != USP_OK) return rc;
  if (want_dq && (rc = launch_dq<D, DT>(p, x, causal, st, row64)) == USP_OK && p.ksplit > 1) rc = launch_reduce_cuts<D, DT>(p, st);
  return rc;
}

}  // namespace usp

static int cuts_of(int32_t n, bool packed) { return (packed || n < 2) ? 1 : (n > 8 ? 8 : n); }

// Keys per work item of the 64-row family's dK/dV launch: 128 (usp_flash_bwd64.hip) or 256 (usp_flash_bwd64u.hip).  A property of
// the call's arguments alone, so that plan_bwd, usp_flash_bwd_workspace_bytes and the launch take the same decision; a launch
// the 64-row family then does not serve runs on another kernel with the plan made here (any plan is valid for any kernel).
// USP_DKDV_KEYS256 / USP_DKDV_KEYS128 force the width.  Otherwise, from what was measured on MI355X (profiles/dkdv_unified.txt;
// the dK/dV launch alone, bf16 causal, medians of 8 alternating rounds, 128 | 256 keys, A/A spread of the 128 arm):
//   B1 S65536 H32/4   8192 items at 256 keys and one head (32 per CU), <= 1024 tiles a head   56.29 | 54.94 ms  (-2.2 %, spread 0.10;
//                                                                                             second box 56.5 | 53.9, -4.6 %)
//   B2 S8192  H16/16  1024 items (4 per CU), <= 128 tiles                                      0.950 | 0.884 ms  (-6.8 %, spread 0.002)
//   B1 S16384 H16/2   1024 items (4 per CU), <= 256 tiles a head                               1.778 | 1.737 ms  (-2.3 %, spread 0.001)
// and, on another box, without the mask (bf16) and in fp16 (causal) -- the other instantiations the rule reaches:
//   full:  B1 S16384 H16/2  3.381 | 3.240 (-4.2 %)   B2 S8192 H16  1.726 | 1.629 (-5.6 %)   B1 S32768 H32/4  27.40 | 25.42 (-7.2 %)
//   fp16:  B1 S16384 H16/2  1.868 | 1.803 (-3.5 %)   B2 S8192 H16  0.982 | 0.916 (-6.7 %)   B1 S65536 H32/4  57.80 | 55.41 (-4.1 %)
//   (A/A spreads 0.012 / 0.0005 / 0.036 and 0.003 / 0.0001 / 0.10 ms)
// -> 256 keys where the launch is one the 64-row family can serve, its 256-key blocks x query heads are at least four per CU and
// its rows at least 8192: the smallest launch measured on either count.  Below that a launch has fewer items than 128-key items
// leave it (half as many, each with 4 - 5 masked tiles at the diagonal instead of 2 - 3) and nothing was measured: 128.  Where
// this picks 256, dkdv_heads_of picks what it picks for 128 (B Hq blocks / 2 >= 2 CUs: its cap, either way).  dkdv_heads in
// {1, 2, 4} at 256 keys, B1 S65536: 55.13 / 54.96 / 55.20 ms; B1 S16384 H16/2: 1.785 / 1.768 / 2.625 -- the causal cap of 2 stays.
static int dkdv_keys_of(const usp_bwd_args* a) {
  if (a->flags & USP_DKDV_KEYS256) return 256;
  if (a->flags & USP_DKDV_KEYS128) return 128;
  if (a->D != 128 || a->seq_q || a->seq_k || (a->flags & (USP_FORCE_WAVE32 | USP_ATTN_SOFTCAP)) || usp::decode_mask(*a).windowed) return 128;
  const int64_t items = (int64_t)a->B * a->Hq * ((a->Sk + 255) / 256);
  return (a->Sq >= 8192 && items >= 4LL * usp::device_cus()) ? 256 : 128;
}

// Query heads of a KV group that ONE dK/dV work item streams into its accumulators (ABI v7: usp_bwd_args.dkdv_heads; a divisor
// of G = Hq / Hkv).  More heads per item: K / V fragments and the epilogue once per run of heads, fewer fp32
// partial slabs (none when the item takes the whole group and nothing is cut) and a shorter reduce; fewer heads: more items,
// which is what balances a causal launch of few (batch, KV head, key block) triangles.  0 = the library decides, from what
// was measured on MI355X (profiles/r06_gqa_loop.txt; dK/dV launch + reduce alone, G = 8):
//   B1 S65536 H32/4 causal   55.1 (1) 54.8 (2) 54.7 (4) 55.2 (8) ms      one KV head of 16384 keys, causal  0.915 (1) 0.896 (2) 1.329 (4) ms
//   B1 S32768 H32/4 causal   14.07    13.91    13.86    14.05            two KV heads, 16384 keys, causal   1.847 (1) 1.798 (2) 1.776 (4) 2.713 (8)
//   one KV head, 8192 rows x 16384 keys, full  0.907 (1) 0.883 (2) 0.871 (4) 1.218 (8)
//   HBM fetch per launch at B1 S65536 (second box: 52.34 / 52.03 / 52.19 ms):  11.4 GB (1)  13.6 GB (2)  33.5 GB (4)
// -> the largest divisor that leaves two items per CU (causal; one when every item is equally long), capped at 4 (eight heads
// per item lose to four even with plenty of items: the per-item saving halves again while every CU's static list shortens to a
// handful of long items) and, for CAUSAL launches, at 2: the 32 workgroups an XCD runs side by side hold 32 consecutive key
// blocks, whose first visible tiles lie up to 62 tiles apart; head after head inside an item that lead adds up, and from three
// heads on the window of Q / dO tiles they stream together (62 tiles x 32 KiB x heads) no longer fits the XCD's 4 MiB L2 -- the
// fetch triples for a time gain inside the noise.  Packed batches keep 1.
static int dkdv_heads_of(const usp_bwd_args* a, int keys) {
  const int G = a->Hq / a->Hkv;
  // an explicit value must divide G whatever G is: MHA (G = 1) accepts 1 only, as usp_hip.h states
  if (a->dkdv_heads > 0) return (G % a->dkdv_heads == 0) ? a->dkdv_heads : -1;
  if (G <= 1) return 1;
  if (a->seq_q || a->seq_k) return 1;
  const int64_t base = (int64_t)a->B * a->Hkv * ((a->Sk + keys - 1) / keys) * cuts_of(a->dkdv_splits, false);
  const bool triangles = usp::decode_mask(*a).causal;
  const int64_t want = (triangles ? 2LL : 1LL) * usp::device_cus();
  int best = 1;
  const int cap = triangles ? 2 : 4;
  for (int g = 2; g <= G && g <= cap; ++g)
    if (G % g == 0 && base * (G / g) >= want) best = g;
  return best;
}

// The plan of a backward call, and with it the layout of its workspace [dK partials | dV partials | dQ partials]:
// (ngrp * qsplit) slabs of ws_rows x Hkv x D each for dK and for dV (none when that is one slab: the whole group in one item
// and no cut), ksplit slabs of B x Sq x Hq x D for dQ (none without a cut).  Needs Hkv > 0 and Hq % Hkv == 0.
struct BwdPlan {
  int keys;                        // keys per dK/dV item of the 64-row family: 128 | 256 (dkdv_keys_of)
  int gsub, ngrp;                  // query heads per dK/dV item (< 1: dkdv_heads does not divide the group), items per KV group
  int qsplit, ksplit;              // cuts of the dK/dV launch, of the dQ launch
  int64_t ws_rows;                 // key rows of a dK/dV slab
  int64_t dkdv_bytes, dq_bytes;
};
static BwdPlan plan_bwd(const usp_bwd_args* a) {
  const bool packed = a->seq_q || a->seq_k;
  BwdPlan pl;
  pl.keys = dkdv_keys_of(a);
  pl.gsub = dkdv_heads_of(a, pl.keys);
  pl.ngrp = pl.gsub < 1 ? 0 : (a->Hq / a->Hkv) / pl.gsub;
  pl.qsplit = cuts_of(a->dkdv_splits, packed);
  pl.ksplit = cuts_of(a->dq_splits, packed);
  pl.ws_rows = packed ? a->total_k : (int64_t)a->B * a->Sk;
  const int64_t slabs = (int64_t)pl.ngrp * pl.qsplit;
  pl.dkdv_bytes = slabs > 1 ? 2 * slabs * pl.ws_rows * a->Hkv * a->D * 4 : 0;
  pl.dq_bytes = pl.ksplit > 1 ? (int64_t)pl.ksplit * a->B * a->Sq * a->Hq * a->D * 4 : 0;
  return pl;
}

extern "C" int64_t usp_flash_bwd_workspace_bytes(const usp_bwd_args* a) {
  if (!a || a->Hkv <= 0 || a->Hq < a->Hkv || a->Hq % a->Hkv != 0) return 0;
  const BwdPlan pl = plan_bwd(a);
  return pl.dkdv_bytes + pl.dq_bytes;
}

// usp_flash_bwd (alibi_slopes == NULL, p_drop == 0, no document array), usp_flash_bwd_alibi, usp_flash_bwd_dropout, usp_flash_bwd_doc
// and usp_flash_bwd_span
static int flash_bwd_call(const usp_bwd_args* a_in, usp::BwdExtras x, void* stream) {
  const usp_bwd_args* a = a_in;
  using namespace usp;
  launch_kinds_reset();
  if (!a || !a->lse || !a->delta) return USP_EINVAL;
  if (int rc = check_force(a->flags)) return rc;
  if ((a->flags & USP_DKDV_KEYS256) && (a->flags & (USP_DKDV_KEYS128 | USP_FORCE_WAVE32))) return USP_EINVAL;
  if ((a->flags & USP_DKDV_KEYS128) && (a->flags & USP_FORCE_WAVE32)) return USP_EINVAL;
  const int skip = a->flags & (USP_BWD_SKIP_DQ | USP_BWD_SKIP_DKDV);
  if (skip == (USP_BWD_SKIP_DQ | USP_BWD_SKIP_DKDV)) return USP_EINVAL;
  if (int rc = check_problem(*a)) return rc;
  if (int rc = check_alibi(*a, x.al.al_slopes, x.al.al_sb)) return rc;
  if (int rc = check_dropout(*a, x.dc, &x.dr)) return rc;
  const BwdDoc& doc = x.doc;
  const bool has_doc = doc.row_lo || doc.key_hi;
  // the dQ launch reads row_lo, the dK/dV launch key_hi: the array of a launch that runs must be there
  if (has_doc && ((!(skip & USP_BWD_SKIP_DQ) && !doc.row_lo) || (!(skip & USP_BWD_SKIP_DKDV) && !doc.key_hi))) return USP_EINVAL;
  // span: the dQ launch reads (row_lo, row_hi), the dK/dV launch (key_lo, key_hi): a launch that runs must have both of its arrays
  // (with them the span's check judges every stride before any decline; it declines all the document's check does)
  const BwdSpan& span = x.span;
  const bool has_span = span.row_hi || span.key_lo;
  if (int rc = check_doc(*a, has_doc && !has_span, doc.row_lo_sb, doc.key_hi_sb)) return rc;
  if (has_span && ((!(skip & USP_BWD_SKIP_DQ) && !(doc.row_lo && span.row_hi)) || (!(skip & USP_BWD_SKIP_DKDV) && !(doc.key_hi && span.key_lo))))
    return USP_EINVAL;
  if (int rc = check_span(*a, has_span, doc.row_lo_sb, doc.key_hi_sb, span.row_hi_sb, span.key_lo_sb)) return rc;
  if (int rc = check_bsp(*a, x.bsp.mask, x.bsp.sb, x.bsp.sh, x.bsp.sr, x.bsp.lists)) return rc;
  const bool has_bsp = x.bsp.mask != nullptr;
  if (has_bsp) x.bsp.layout = block_lists(a->B, a->Hq, (a->Sq + 127) / 128, (a->Sk + 127) / 128);   // once per call
  if (!a->dout.ptr || !a->q.ptr || !a->k.ptr || !a->v.ptr) return USP_EINVAL;
  const bool packed = a->seq_q != nullptr || a->seq_k != nullptr;
  if (packed && !(a->seq_q && a->seq_k && a->total_k > 0)) return USP_EINVAL;
  // an fp32 tensor may be absent only if its 16-bit final output is given and nothing is accumulated
  auto need32 = [](const usp_tensor& t32, const usp_tensor& t16, int accum) { return !t16.ptr || accum; };
  const bool want_dq = !(skip & USP_BWD_SKIP_DQ), want_dkdv = !(skip & USP_BWD_SKIP_DKDV);   // (a skipped launch needs no outputs)
  if ((want_dq && need32(a->dq, a->dq16, a->accum_dq) && !a->dq.ptr) || (want_dkdv && need32(a->dk, a->dk16, a->accum_dk) && !a->dk.ptr) ||
      (want_dkdv && need32(a->dv, a->dv16, a->accum_dv) && !a->dv.ptr))
    return USP_EINVAL;
  auto ok32 = [](const usp_tensor& t) { return !t.ptr || tensor_aligned(t, 16, 4); };      // optional fp32 / 16-bit outputs
  auto ok16 = [](const usp_tensor& t) { return !t.ptr || tensor_aligned(t, 8, 4); };
  if (!tensor_aligned(a->dout, 16, 8) || !tensor_aligned(a->q, 16, 8) || !tensor_aligned(a->k, 16, 8) || !tensor_aligned(a->v, 16, 8) ||
      !ok32(a->dq) || !ok32(a->dk) || !ok32(a->dv) || !ok16(a->dq16) || !ok16(a->dk16) || !ok16(a->dv16))
    return USP_EUNSUPPORTED;
  const Mask mask = decode_mask(*a);
  if (packed && (mask.windowed || mask.shifted)) return USP_EUNSUPPORTED;        // dense launches only
  if (a->dq_splits < 0 || a->dq_splits > 8 || a->dkdv_splits < 0 || a->dkdv_splits > 8) return USP_EINVAL;
  usp_bwd_args uncut;                              // a document launch is served uncut (usp_hip.h): the plan of the same call without cuts
  if (has_doc || has_span || has_bsp) { uncut = *a; uncut.dq_splits = 0; uncut.dkdv_splits = 0; a = &uncut; }
  const BwdPlan plan = plan_bwd(a);
  if (a->dkdv_heads < 0 || plan.gsub < 1) return USP_EINVAL;       // (not a divisor of Hq / Hkv)
  BwdArgsSC p;
  p.dout = (const char*)a->dout.ptr; p.q = (const char*)a->q.ptr;
  p.k = (const char*)a->k.ptr; p.v = (const char*)a->v.ptr;
  p.lse = a->lse; p.delta = a->delta;
  p.dq = (float*)a->dq.ptr; p.dk = (float*)a->dk.ptr; p.dv = (float*)a->dv.ptr;
  p.do_sb = a->dout.stride_b; p.do_ss = a->dout.stride_s; p.do_sh = a->dout.stride_h;
  p.q_sb = a->q.stride_b; p.q_ss = a->q.stride_s; p.q_sh = a->q.stride_h;
  p.k_sb = a->k.stride_b; p.k_ss = a->k.stride_s; p.k_sh = a->k.stride_h;
  p.v_sb = a->v.stride_b; p.v_ss = a->v.stride_s; p.v_sh = a->v.stride_h;
  p.lse_sb = a->lse_stride_b; p.lse_sh = a->lse_stride_h;
  p.dl_sb = a->delta_stride_b; p.dl_sh = a->delta_stride_h;
  p.dq_sb = a->dq.stride_b; p.dq_ss = a->dq.stride_s; p.dq_sh = a->dq.stride_h;
  p.dk_sb = a->dk.stride_b; p.dk_ss = a->dk.stride_s; p.dk_sh = a->dk.stride_h;
  p.dv_sb = a->dv.stride_b; p.dv_ss = a->dv.stride_s; p.dv_sh = a->dv.stride_h;
  p.B = a->B; p.Sq = a->Sq; p.Sk = a->Sk; p.Hq = a->Hq; p.Hkv = a->Hkv; p.G = a->Hq / a->Hkv;
  p.nblk = 0;
  mask.store(p);
  p.scale = a->softmax_scale;
  p.scale_log2 = a->softmax_scale * kLog2e;
  p.accum_dq = a->accum_dq ? 1 : 0; p.accum_dk = a->accum_dk ? 1 : 0; p.accum_dv = a->accum_dv ? 1 : 0;
  p.dq16 = (char*)a->dq16.ptr; p.dk16 = (char*)a->dk16.ptr; p.dv16 = (char*)a->dv16.ptr;
  p.dq16_sb = a->dq16.stride_b; p.dq16_ss = a->dq16.stride_s; p.dq16_sh = a->dq16.stride_h;
  p.dk16_sb = a->dk16.stride_b; p.dk16_ss = a->dk16.stride_s; p.dk16_sh = a->dk16.stride_h;
  p.dv16_sb = a->dv16.stride_b; p.dv16_ss = a->dv16.stride_s; p.dv16_sh = a->dv16.stride_h;
  p.seq_q = a->seq_q; p.seq_k = a->seq_k;
  p.sched = packed ? a->sched : nullptr;
  p.sched_lds = 0;
  p.interleave = (a->flags & USP_LAUNCH_INTERLEAVE) ? 1 : 0;
  p.walk_g = p.G;                                 // a KV group's heads side by side in the item walk
  p.wide16 = 0;                                   // (set by the 64-row launches for their own copy)
  p.ws_rows = plan.ws_rows;
  if (packed) {
    p.do_sb = p.q_sb = p.k_sb = p.v_sb = p.lse_sb = p.dl_sb = 0;
    p.dq_sb = p.dk_sb = p.dv_sb = p.dq16_sb = p.dk16_sb = p.dv16_sb = 0;
  }
  // Workspace present and large enough: the dK/dV items of plan.gsub query heads each and / or the requested cuts, partials
  // summed afterwards; otherwise neither (the whole KV group inside one workgroup, one item per key block) -- results are
  // identical up to fp32 summation order either way.
  p.split = 0; p.qsplit = 1; p.ksplit = 1; p.nslab = 1; p.ws_dk = nullptr; p.ws_dv = nullptr; p.ws_dq = nullptr;
  p.gsub = p.G; p.ngrp = 1;
  const int64_t need = plan.dkdv_bytes + plan.dq_bytes;
  if (need > 0 && a->workspace && a->workspace_bytes >= need && aligned(a->workspace, 16)) {
    if (plan.dkdv_bytes > 0) {
      p.split = 1;
      p.gsub = plan.gsub; p.ngrp = plan.ngrp; p.qsplit = plan.qsplit;
      p.nslab = p.ngrp * p.qsplit;
      p.ws_dk = (float*)a->workspace;
      p.ws_dv = p.ws_dk + plan.dkdv_bytes / 8;
    }
    p.ksplit = plan.ksplit;
    if (p.ksplit > 1) p.ws_dq = (float*)((char*)a->workspace + plan.dkdv_bytes);
  }
  x.al.al_diag = alibi_diag(*a);
  const int force = a->flags & (USP_FORCE_ROW64 | USP_FORCE_WAVE32 | USP_DKDV_KEYS256 | USP_DKDV_KEYS128);
  return with_head_dim_dtype(a->D, a->dtype, [&](auto d, auto dt) {
    return launch_bwd<decltype(d)::value, decltype(dt)::value>(p, x, mask.causal, (hipStream_t)stream, force, skip, plan.keys);
  });
}

extern "C" int usp_flash_bwd(const usp_bwd_args* a, void* stream) { return flash_bwd_call(a, usp::BwdExtras{}, stream); }

extern "C" int usp_flash_bwd_alibi(const usp_bwd_args* a, const float* alibi_slopes, int64_t alibi_stride_b, void* stream) {
  usp::BwdExtras x;
  x.al.al_slopes = alibi_slopes; x.al.al_sb = alibi_stride_b;
  return flash_bwd_call(a, x, stream);
}

extern "C" int usp_flash_bwd_dropout(const usp_bwd_args* a, float p_drop, uint64_t seed, int32_t row0, int32_t key0, int32_t head0,
                                     void* stream) {
  usp::BwdExtras x;
  x.dc = usp::DropoutCall{p_drop, seed, row0, key0, head0};
  return flash_bwd_call(a, x, stream);
}

extern "C" int usp_flash_bwd_doc(const usp_bwd_args* a, const int32_t* row_lo, int64_t row_lo_stride_b, const int32_t* key_hi,
                                 int64_t key_hi_stride_b, void* stream) {
  const bool any = row_lo || key_hi;
  usp::BwdExtras x;
  x.doc = usp::BwdDoc{row_lo, key_hi, any ? row_lo_stride_b : 0, any ? key_hi_stride_b : 0};
  return flash_bwd_call(a, x, stream);
}

extern "C" int usp_flash_bwd_span(const usp_bwd_args* a, const int32_t* row_lo, int64_t row_lo_stride_b, const int32_t* row_hi,
                                  int64_t row_hi_stride_b, const int32_t* key_lo, int64_t key_lo_stride_b, const int32_t* key_hi,
                                  int64_t key_hi_stride_b, void* stream) {
  const bool any = row_lo || key_hi, any_span = row_hi || key_lo;    // row_hi == key_lo == NULL: exactly usp_flash_bwd_doc
  usp::BwdExtras x;
  x.doc = usp::BwdDoc{row_lo, key_hi, any ? row_lo_stride_b : 0, any ? key_hi_stride_b : 0};
  x.span = usp::BwdSpan{row_hi, key_lo, any_span ? row_hi_stride_b : 0, any_span ? key_lo_stride_b : 0};
  return flash_bwd_call(a, x, stream);
}

extern "C" int usp_flash_bwd_bsp(const usp_bwd_args* a, const void* mask, int64_t mask_stride_b, int64_t mask_stride_h,
                                 int64_t mask_stride_row, void* lists, void* stream) {
  usp::BwdExtras x;                                                   // mask == NULL: exactly usp_flash_bwd
  if (mask) x.bsp = usp::BspCall{mask, mask_stride_b, mask_stride_h, mask_stride_row, (int*)lists};
  return flash_bwd_call(a, x, stream);
}
