// Blockwise flash-attention backward for gfx950.  C ABI: usp_flash_bwd (include/usp_hip.h).
// Replaces the reference's `bwd-only` block kernel (yunchang/kernels/attention.py:205-250) plus the
// fp32 accumulation the ring schedules do on its results (zigzag_ring_flash_attn.py:147-170).
//
// Two launches, no atomics, deterministic:
//   dQ     (flash_bwd_kernel)      : workgroup = 8 waves x 32 query rows; streams K,V tiles (64 keys) through LDS.
//                                    lane owns a query row:  S^T = K Q^T, dP^T = V dO^T, dQ^T += K^T dS^T
//   dK, dV (flash_bwd_dkdv_kernel) : workgroup = 8 waves, 128 keys, two roles (below); the one-wave-per-SIMD form of it
//                                    lives in usp_flash_bwd64.hip and serves the dense D = 128 launches.
// Both are one engine: two LDS tiles X1,X2 (row-major, 16-byte-slot XOR swizzle chosen so that
// BOTH ds_read_b128 row reads and ds_read_b64_tr_b16 column reads are bank-conflict free), two
// register-resident fragment sets R1,R2, S = X1 R1^T, T = X2 R2^T, and tr-read "X^T" operands for
// the gradient MFMAs.  As in the forward, no cross-lane shuffle is needed for P / dS: the k-step
// order of the gradient MFMAs is defined as the order the S accumulator holds rows.
#include <stdlib.h>

#include <type_traits>

#include "usp_bwd_params.hpp"
#include "usp_common.hpp"
#include "usp_hip.h"

namespace usp {

// SC: logit soft-capping (USP_ATTN_SOFTCAP; PA = BwdArgsSC): with t = tanh(S/cap) of the raw (masked) score,
// P = exp2(cap*log2e*t - lse2) (0 where masked) and dS = P (dP - delta) (1 - t^2), in place; the epilogue's `scale` is
// unchanged.  The body is shared by two __global__ templates so that the kernel without softcap keeps its symbol name
// and machine code.

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_kernel(
    const BwdParams p_in) {
  constexpr bool SC = false;
  constexpr float sc_cl2 = 0.f, sc_k2 = 0.f;
#include "usp_flash_bwd_dq_body.inc"
}

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_softcap_kernel(const BwdArgsSC p_in) {
  constexpr bool SC = true;
  const float sc_cl2 = p_in.cap_log2, sc_k2 = p_in.tanh_k2;
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
  constexpr bool SC = false;
  constexpr float sc_cl2 = 0.f, sc_k2 = 0.f;
#include "usp_flash_bwd_dkdv_body.inc"
}

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_dkdv_softcap_kernel(const BwdArgsSC p_in) {
  constexpr bool SC = true;
  const float sc_cl2 = p_in.cap_log2, sc_k2 = p_in.tanh_k2;
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

template <int D, int DT>
static int launch_bwd(BwdArgsSC p, bool causal, hipStream_t st, int force, int skip) {
  constexpr size_t lds0 = 2 * (2 * kTile * D * 2);
  // dK,dV
  // persistent launches: one workgroup per CU (both kernels fit once per CU), each walks n_items / grid items
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  static const bool persist = [] { const char* e = getenv("USP_BWD_PERSIST"); return !(e && e[0] == '0'); }();
  p.nblk = (p.Sk + 127) / 128;
  p.n_items = p.B * p.Hkv * p.nblk * p.ngrp * p.qsplit;
  const bool pers = (persist || p.sched) && !p.interleave;
  int grid = (pers && p.n_items > cus) ? cus : p.n_items;
  const size_t qx = p.sched ? 16 : 0;            // LDS for the item queue's two slots
  // dK/dV: the one-wave-per-SIMD kernel (4 waves x 64 keys, usp_flash_bwd64.hip) where it applies; USP_BWD_WAVES=8 forces
  // the 8-wave kernel below
  // (per call: `force` = USP_FORCE_ROW64 / USP_FORCE_WAVE32, include/usp_hip.h)
  static const int forced_env = [] { const char* e = getenv("USP_BWD_WAVES"); return e ? atoi(e) : 0; }();
  const int forced_waves = (force & USP_FORCE_WAVE32) ? 8 : ((force & USP_FORCE_ROW64) ? 0 : forced_env);
  if ((force & USP_FORCE_ROW64) && !(D == 128 && ((skip & USP_BWD_SKIP_DKDV) || dkdv64_serves(p, DT)) && ((skip & USP_BWD_SKIP_DQ) || dq64_serves(p))))
    return USP_EUNSUPPORTED;     // (only the launches that will run have to be served)
  bool dkdv_done = (skip & USP_BWD_SKIP_DKDV) != 0;
  const bool row64_ok = !p.cap_on;               // the 64-row kernels' hand-pinned pipelines have no softcap step
  if (!dkdv_done && D == 128 && forced_waves != 8 && row64_ok) {
    int rc64 = USP_ELAUNCH;
    if (launch_dkdv64(p, DT, causal, st, &rc64)) {
      if (rc64 != USP_OK) return rc64;
      dkdv_done = true;
      launch_kinds_note(USP_KIND_DKDV_ROW64);
    }
  }
  if (!dkdv_done) {
    // the 8-wave dK/dV kernel addresses the Q / dO tiles of a head by a 32-bit byte offset from the head's first row
    if ((int64_t)p.Sq * p.q_ss * 2 >= (1LL << 31) || (int64_t)p.Sq * p.do_ss * 2 >= (1LL << 31)) return USP_EUNSUPPORTED;
  {
    constexpr size_t lds2 = 3 * (2 * kTile * D * 2 + 2 * kTile * 4) + 4 * 2 * 4096;
    p.sched_lds = (int)lds2;
    const BwdParams pb = p;
    if (p.cap_on) {
      if (causal)
        hipLaunchKernelGGL((flash_bwd_dkdv_softcap_kernel<D, DT, true>), dim3(grid), dim3(512), lds2 + qx, st, p);
      else
        hipLaunchKernelGGL((flash_bwd_dkdv_softcap_kernel<D, DT, false>), dim3(grid), dim3(512), lds2 + qx, st, p);
    } else if (causal)
      hipLaunchKernelGGL((flash_bwd_dkdv_kernel<D, DT, true>), dim3(grid), dim3(512), lds2 + qx, st, pb);
    else
      hipLaunchKernelGGL((flash_bwd_dkdv_kernel<D, DT, false>), dim3(grid), dim3(512), lds2 + qx, st, pb);
    launch_kinds_note(USP_KIND_DKDV_WAVE8);
  }
  }
  if (hipGetLastError() != hipSuccess) return USP_ELAUNCH;
  if (p.split && !(skip & USP_BWD_SKIP_DKDV)) {
    const int64_t items = (int64_t)p.B * p.Sk * p.Hkv * (D / 4);
    int64_t rg = (items + 255) / 256;
    rg = rg > 2048 ? 2048 : rg;
    const BwdParams pb = p;
    hipLaunchKernelGGL((reduce_heads_kernel<D, DT>), dim3((int)rg), dim3(256), 0, st, pb);
    if (hipGetLastError() != hipSuccess) return USP_ELAUNCH;
    launch_kinds_note(USP_KIND_REDUCE_HEADS);
  }
  if (skip & USP_BWD_SKIP_DQ) return USP_OK;
  // dQ: the one-wave-per-SIMD kernel (4 waves x 64 query rows, usp_flash_bwd_dq64.hip) where it applies
  static const int forced_dq_env = [] { const char* e = getenv("USP_BWD_DQ_WAVES"); return e ? atoi(e) : 0; }();
  const int forced_dq = force ? 0 : forced_dq_env;
  if (D == 128 && forced_waves != 8 && forced_dq != 8 && row64_ok) {
    int rc64 = USP_ELAUNCH;
    if (launch_dq64(p, DT, causal, st, &rc64)) {
      if (rc64 != USP_OK) return rc64;
      launch_kinds_note(USP_KIND_DQ_ROW64);
      if (p.ksplit > 1) {          // same stream: the cuts' partials are complete when this starts
        const int64_t items = (int64_t)p.B * p.Sq * p.Hq * (D / 4);
        int64_t rg = (items + 255) / 256;
        rg = rg > 2048 ? 2048 : rg;
        const BwdParams pb = p;
        hipLaunchKernelGGL((reduce_cuts_kernel<D, DT>), dim3((int)rg), dim3(256), 0, st, pb);
        launch_kinds_note(USP_KIND_REDUCE_CUTS);
      }
      return hipGetLastError() == hipSuccess ? USP_OK : USP_ELAUNCH;
    }
  }
  p.nblk = (p.Sq + 255) / 256;
  p.n_items = p.B * p.Hq * p.nblk * p.ksplit;
  grid = (pers && p.n_items > cus) ? cus : p.n_items;
  p.sched_lds = (int)lds0;
  const BwdParams pb = p;
  if (p.cap_on) {
    if (causal)
      hipLaunchKernelGGL((flash_bwd_softcap_kernel<D, DT, true>), dim3(grid), dim3(512), lds0 + qx, st, p);
    else
      hipLaunchKernelGGL((flash_bwd_softcap_kernel<D, DT, false>), dim3(grid), dim3(512), lds0 + qx, st, p);
  } else if (causal)
    hipLaunchKernelGGL((flash_bwd_kernel<D, DT, true>), dim3(grid), dim3(512), lds0 + qx, st, pb);
  else
    hipLaunchKernelGGL((flash_bwd_kernel<D, DT, false>), dim3(grid), dim3(512), lds0 + qx, st, pb);
  if (hipGetLastError() != hipSuccess) return USP_ELAUNCH;
  launch_kinds_note(USP_KIND_DQ_WAVE8);
  if (p.ksplit > 1) {            // same stream: the partials are complete when this starts
    const int64_t items = (int64_t)p.B * p.Sq * p.Hq * (D / 4);
    int64_t rg = (items + 255) / 256;
    rg = rg > 2048 ? 2048 : rg;
    hipLaunchKernelGGL((reduce_cuts_kernel<D, DT>), dim3((int)rg), dim3(256), 0, st, pb);
    launch_kinds_note(USP_KIND_REDUCE_CUTS);
  }
  return hipGetLastError() == hipSuccess ? USP_OK : USP_ELAUNCH;
}

static bool ok16(const usp_tensor& t, int esize) {
  const int m = 16 / esize;
  return t.ptr && (reinterpret_cast<uintptr_t>(t.ptr) & 15) == 0 && t.stride_b % m == 0 &&
         t.stride_s % m == 0 && t.stride_h % m == 0;
}

}  // namespace usp

static int64_t ws_rows_of(const usp_bwd_args* a) {
  return (a->seq_q || a->seq_k) ? a->total_k : (int64_t)a->B * a->Sk;
}

static int cuts_of(int32_t n, bool packed) { return (packed || n < 2) ? 1 : (n > 8 ? 8 : n); }

static int device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  return cus;
}

// Query heads of a KV group that ONE dK/dV work item streams into its accumulators (ABI v7: usp_bwd_args.dkdv_heads; a divisor
// of G = Hq / Hkv).  More heads per item: K / V fragments, their pre-scale and the epilogue once per run of heads, fewer fp32
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
// fetch triples for a time gain inside the noise.  Packed batches keep 1.  USP_BWD_GSUB=n (read once) overrides the automatic
// choice for A/B runs.
static int dkdv_heads_of(const usp_bwd_args* a) {
  const int G = a->Hq / a->Hkv;
  // an explicit value must divide G whatever G is: MHA (G = 1) accepts 1 only, as usp_hip.h states
  if (a->dkdv_heads > 0) return (G % a->dkdv_heads == 0) ? a->dkdv_heads : -1;
  if (G <= 1) return 1;
  if (a->seq_q || a->seq_k) return 1;
  static const int forced = [] { const char* e = getenv("USP_BWD_GSUB"); return e ? atoi(e) : 0; }();
  if (forced > 0) {
    int g = forced > G ? G : forced;
    while (G % g != 0) --g;
    return g;
  }
  const int64_t base = (int64_t)a->B * a->Hkv * ((a->Sk + 127) / 128) * cuts_of(a->dkdv_splits, false);
  const bool triangles = a->causal || ((a->flags & USP_ATTN_WINDOW) && a->window_right >= 0);
  const int64_t want = (triangles ? 2LL : 1LL) * device_cus();
  int best = 1;
  const int cap = triangles ? 2 : 4;
  for (int g = 2; g <= G && g <= cap; ++g)
    if (G % g == 0 && base * (G / g) >= want) best = g;
  return best;
}

// [dK partials | dV partials | dQ partials]: ((G / dkdv_heads) * dkdv_splits) slabs of ws_rows x Hkv x D each for dK and for dV
// (none when that is one slab: the whole group in one item and no cut), dq_splits slabs of B x Sq x Hq x D for dQ (none without a cut)
static int64_t dkdv_part_bytes(const usp_bwd_args* a) {
  const int gsub = dkdv_heads_of(a);
  if (gsub < 1) return 0;
  const int64_t slabs = (int64_t)((a->Hq / a->Hkv) / gsub) * cuts_of(a->dkdv_splits, a->seq_q || a->seq_k);
  return slabs > 1 ? 2 * slabs * ws_rows_of(a) * a->Hkv * a->D * 4 : 0;
}

extern "C" int64_t usp_flash_bwd_workspace_bytes(const usp_bwd_args* a) {
  if (!a || a->Hkv <= 0 || a->Hq < a->Hkv || a->Hq % a->Hkv != 0) return 0;
  const int nq = cuts_of(a->dq_splits, a->seq_q || a->seq_k);
  return dkdv_part_bytes(a) + (nq > 1 ? (int64_t)nq * a->B * a->Sq * a->Hq * a->D * 4 : 0);
}

extern "C" int usp_flash_bwd(const usp_bwd_args* a, void* stream) {
  using namespace usp;
  launch_kinds_reset();
  if (!a || !a->lse || !a->delta) return USP_EINVAL;
  const int force = a->flags & (USP_FORCE_ROW64 | USP_FORCE_WAVE32);
  if (force == (USP_FORCE_ROW64 | USP_FORCE_WAVE32)) return USP_EINVAL;
  const int skip = a->flags & (USP_BWD_SKIP_DQ | USP_BWD_SKIP_DKDV);
  if (skip == (USP_BWD_SKIP_DQ | USP_BWD_SKIP_DKDV)) return USP_EINVAL;
  if (a->dtype != USP_BF16 && a->dtype != USP_FP16) return USP_EINVAL;
  if (a->B <= 0 || a->Sq <= 0 || a->Sk <= 0 || a->Hq <= 0 || a->Hkv <= 0) return USP_EINVAL;
  if (!(a->softmax_scale > 0.f)) return USP_EINVAL;
  const bool has_cap = (a->flags & USP_ATTN_SOFTCAP) != 0;     // (the field is read only with the bit)
  if (has_cap && !(__builtin_isfinite(a->softcap) && a->softcap > 0.f)) return USP_EINVAL;
  if (has_cap && (force & USP_FORCE_ROW64)) return USP_EUNSUPPORTED;   // the 64-row family declines softcap
  if (a->D != 32 && a->D != 64 && a->D != 128) return USP_EUNSUPPORTED;
  if (a->Hq % a->Hkv != 0) return USP_EUNSUPPORTED;
  if (!a->dout.ptr || !a->q.ptr || !a->k.ptr || !a->v.ptr) return USP_EINVAL;
  const bool packed = a->seq_q != nullptr || a->seq_k != nullptr;
  if (packed && !(a->seq_q && a->seq_k && a->total_k > 0)) return USP_EINVAL;
  // an fp32 tensor may be absent only if its 16-bit final output is given and nothing is accumulated
  auto need32 = [](const usp_tensor& t32, const usp_tensor& t16, int accum) { return !t16.ptr || accum; };
  const bool want_dq = !(a->flags & USP_BWD_SKIP_DQ), want_dkdv = !(a->flags & USP_BWD_SKIP_DKDV);   // (a skipped launch needs no outputs)
  if ((want_dq && need32(a->dq, a->dq16, a->accum_dq) && !a->dq.ptr) || (want_dkdv && need32(a->dk, a->dk16, a->accum_dk) && !a->dk.ptr) ||
      (want_dkdv && need32(a->dv, a->dv16, a->accum_dv) && !a->dv.ptr))
    return USP_EINVAL;
  auto ok32 = [](const usp_tensor& t) { return !t.ptr || ok16(t, 4); };
  auto okh = [](const usp_tensor& t) {
    return !t.ptr || ((reinterpret_cast<uintptr_t>(t.ptr) & 7) == 0 && t.stride_b % 4 == 0 &&
                      t.stride_s % 4 == 0 && t.stride_h % 4 == 0);
  };
  if (!ok16(a->dout, 2) || !ok16(a->q, 2) || !ok16(a->k, 2) || !ok16(a->v, 2) || !ok32(a->dq) ||
      !ok32(a->dk) || !ok32(a->dv) || !okh(a->dq16) || !okh(a->dk16) || !okh(a->dv16))
    return USP_EUNSUPPORTED;
  // sliding window (flash-attn's window_size), as in usp_flash_fwd: causal caps the right bound at 0, a right bound is
  // the causal limit with a shifted offset, a left bound is a second mask term + a shorter streamed range
  const bool has_win = (a->flags & USP_ATTN_WINDOW) != 0;
  const int wl = has_win ? a->window_left : -1;
  const int wr = a->causal ? 0 : (has_win ? a->window_right : -1);
  if ((a->seq_q || a->seq_k) && (wl >= 0 || wr > 0)) return USP_EUNSUPPORTED;       // dense launches only
  if (a->dq_splits < 0 || a->dq_splits > 8 || a->dkdv_splits < 0 || a->dkdv_splits > 8) return USP_EINVAL;
  if (a->dkdv_heads < 0 || dkdv_heads_of(a) < 1) return USP_EINVAL;       // (not a divisor of Hq / Hkv)
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
  p.causal_off = a->Sk - a->Sq + (wr > 0 ? wr : 0);
  p.win_on = wl >= 0 ? 1 : 0; p.win_lo = a->Sk - a->Sq - (wl >= 0 ? wl : 0);
  p.scale = a->softmax_scale;
  p.scale_log2 = a->softmax_scale * kLog2e;
  p.cap_on = has_cap ? 1 : 0;
  p.cap_log2 = has_cap ? a->softcap * kLog2e : 0.f;
  p.tanh_k2 = has_cap ? 2.f * a->softmax_scale * kLog2e / a->softcap : 0.f;
  p.accum_dq = a->accum_dq ? 1 : 0; p.accum_dk = a->accum_dk ? 1 : 0; p.accum_dv = a->accum_dv ? 1 : 0;
  p.dq16 = (char*)a->dq16.ptr; p.dk16 = (char*)a->dk16.ptr; p.dv16 = (char*)a->dv16.ptr;
  p.dq16_sb = a->dq16.stride_b; p.dq16_ss = a->dq16.stride_s; p.dq16_sh = a->dq16.stride_h;
  p.dk16_sb = a->dk16.stride_b; p.dk16_ss = a->dk16.stride_s; p.dk16_sh = a->dk16.stride_h;
  p.dv16_sb = a->dv16.stride_b; p.dv16_ss = a->dv16.stride_s; p.dv16_sh = a->dv16.stride_h;
  // GQA head split: with a workspace, every query head of a KV group gets its own workgroups and the
  // per-head partials are summed afterwards; without one the group's heads are looped inside a workgroup.
  p.seq_q = a->seq_q; p.seq_k = a->seq_k;
  p.sched = packed ? a->sched : nullptr;
  p.sched_lds = 0;
  p.interleave = (a->flags & USP_LAUNCH_INTERLEAVE) ? 1 : 0;
  {   // USP_ITEM_GROUP=0 (read once): the head-major item walk of rounds 1-5 instead of a KV group's heads side by side
    static const bool group_heads = [] { const char* e = getenv("USP_ITEM_GROUP"); return !(e && e[0] == '0'); }();
    p.walk_g = group_heads ? p.G : 1;
  }
  p.wide16 = 0;                                   // (set by the 64-row launches for their own copy)
  p.ws_rows = ws_rows_of(a);
  if (packed) {
    p.do_sb = p.q_sb = p.k_sb = p.v_sb = p.lse_sb = p.dl_sb = 0;
    p.dq_sb = p.dk_sb = p.dv_sb = p.dq16_sb = p.dk16_sb = p.dv16_sb = 0;
  }
  // Workspace present and large enough: the dK/dV items of dkdv_heads_of() query heads each and / or the requested cuts;
  // otherwise neither (the whole KV group inside one workgroup, one item per key block) -- results are identical up to fp32
  // summation order either way.
  const int64_t need = usp_flash_bwd_workspace_bytes(a);
  p.split = 0; p.qsplit = 1; p.ksplit = 1; p.nslab = 1; p.ws_dk = nullptr; p.ws_dv = nullptr; p.ws_dq = nullptr;
  p.gsub = p.G; p.ngrp = 1;
  if (need > 0 && a->workspace && a->workspace_bytes >= need &&
      (reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0) {
    const int64_t part = dkdv_part_bytes(a);
    if (part > 0) {
      p.split = 1;
      p.gsub = dkdv_heads_of(a);
      p.ngrp = p.G / p.gsub;
      p.qsplit = cuts_of(a->dkdv_splits, packed);
      p.nslab = p.ngrp * p.qsplit;
      p.ws_dk = (float*)a->workspace;
      p.ws_dv = p.ws_dk + part / 8;
    }
    p.ksplit = cuts_of(a->dq_splits, packed);
    if (p.ksplit > 1) p.ws_dq = (float*)((char*)a->workspace + part);
  }
  hipStream_t st = (hipStream_t)stream;
  const bool causal = wr >= 0;                    // (a->causal, or a right window bound)
  switch (a->D * 2 + a->dtype) {
    case 64: return launch_bwd<32, 0>(p, causal, st, force, skip);
    case 65: return launch_bwd<32, 1>(p, causal, st, force, skip);
    case 128: return launch_bwd<64, 0>(p, causal, st, force, skip);
    case 129: return launch_bwd<64, 1>(p, causal, st, force, skip);
    case 256: return launch_bwd<128, 0>(p, causal, st, force, skip);
    case 257: return launch_bwd<128, 1>(p, causal, st, force, skip);
  }
  return USP_EUNSUPPORTED;
}
