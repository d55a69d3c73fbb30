// Blockwise flash-attention forward for gfx950 with the ring LSE-merge fused into the epilogue.
// C ABI: usp_flash_fwd (include/usp_hip.h).  Replaces the reference's `fwd-only` block kernel
// (yunchang/kernels/attention.py:44-136) and update_out_and_lse (yunchang/ring/utils.py:10-51).
//
// Structure (one workgroup = 8 waves = 256 query rows of one (batch, head); KV tile = 64 keys):
//   * "fully swapped" MFMA orientation: S^T = K Q^T and O^T = V^T P^T with
//     v_mfma_f32_32x32x16, so that every lane owns ONE query row (q = lane & 31) in both
//     accumulators; the two half-waves hold complementary key / dim subsets.  Row max / sum /
//     rescale / LSE merge are therefore lane-local (+ one v_permlane32_swap per row statistic).
//   * Q fragments live in registers for the whole kernel (B operand of K Q^T).
//   * K tile in LDS row-major with a 16-byte-slot XOR swizzle -> conflict-free ds_read_b128.
//   * V tile in LDS as [4 keys][32 dims] 256-byte blocks -> ds_read_b64_tr_b16 delivers the
//     A operand of V^T P^T directly; one block = exactly one LDS bank row per half-wave.
//   * P needs no cross-lane shuffle: the key order of each PV k-step is DEFINED as the order in
//     which the S^T accumulator holds keys, and V is read in that same order.
//   * K/V tiles are double-buffered in LDS and filled by LDS-DMA (buffer_load ... lds) one tile (V) /
//     two tiles (K) ahead: no staging registers, no ds_write; one barrier per tile.
//   * exp2 with softmax_scale*log2(e) folded into one FMA per score.
#include "usp_fwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

// NWAVES waves per workgroup, 32 query rows each: 8 (one 256-row workgroup per CU) or 4 (two 128-row
// workgroups per CU: half the causal diagonal waste, and the two workgroups desynchronise).
// Every kernel of the family is the shared body (usp_flash_fwd_body.inc) under a __global__ template that gives it a name, an
// argument block `p_in`, WIN and CAUSAL; the body derives its other switches from the block's type ("How a kernel
// variant is declared").  The kernels here and the variants in usp_flash_fwd_{alibi,dropout,sink,maxl,doc,span,bsp}.hip:
//   flash_fwd_kernel<.., false>  the plain argument block.  The K-split form is an instantiation of its own, <.., true> on
//     FwdArgsT<true>: the plain kernels sit on the register cliff (256 VGPRs), and with the split code compiled in
//     unconditionally hipcc spilled 16 more bytes in them.
//   flash_fwd_window_kernel  WIN: a left window bound (USP_ATTN_WINDOW with window_left >= 0) on the split block.  The tiles no
//     bound cuts for a wave take the hand-pinned main loop (rotated tile walk, see the body); in the other kernels a left bound
//     -- softcap launches still carry one -- sends every tile through the generic loop.
//   flash_fwd_softcap_kernel  FwdArgsSC, logit soft-capping (USP_ATTN_SOFTCAP): every tile takes the generic loop, which replaces
//     the raw score tile by cap*tanh(S/cap) (in exp2 units) BEFORE the mask -- tanh(-inf) = -1, a key masked first would keep a
//     weight -- and runs the online softmax with c = 1.
template <int D, int DT, bool CAUSAL, int NWAVES, bool KS = false>
__global__ __launch_bounds__(64 * NWAVES, 2) void flash_fwd_kernel(const FwdArgsT<KS> p_in) {
  constexpr bool WIN = false;
#include "usp_flash_fwd_body.inc"
}

template <int D, int DT, bool CAUSAL, int NWAVES>
__global__ __launch_bounds__(64 * NWAVES, 2) void flash_fwd_window_kernel(const FwdArgsT<true> p_in) {
  constexpr bool WIN = true;
#include "usp_flash_fwd_body.inc"
}

template <int D, int DT, bool CAUSAL, int NWAVES>
__global__ __launch_bounds__(64 * NWAVES, 2) void flash_fwd_softcap_kernel(const FwdArgsSC p_in) {
  constexpr bool WIN = false;
#include "usp_flash_fwd_body.inc"
}

// Combines the partial results of a K-split launch: per query row, the `n` cuts' normalised partials (fp32) and
// LSEs [+ the running result when merge_in] -> what ONE launch would have left behind: lse, and the row in 16 bits
// (final rows) or fp32 (the others).  HBM-bound: one thread per 4 consecutive head-dim elements of a row.
template <int DT>
__global__ __launch_bounds__(256) void split_merge_kernel(const FwdArgsT<true> p, int D) {
  using E = Elem<DT>;
  const int d4 = D >> 2;
  const int64_t total = (int64_t)p.B * p.Sq * p.Hq * d4;
  const int64_t slot_o = (int64_t)p.B * p.Sq * p.Hq * D, slot_l = (int64_t)p.B * p.Hq * p.Sq;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % d4);
    int64_t r = i / d4;
    const int h = (int)(r % p.Hq); r /= p.Hq;
    const int s = (int)(r % p.Sq);
    const int b = (int)(r / p.Sq);
    const int64_t l_idx = ((int64_t)b * p.Hq + h) * p.Sq + s;
    const int64_t o_idx = (((int64_t)b * p.Sq + s) * p.Hq + h) * D + 4 * c4;
    float* lse_p = p.lse + b * p.lse_sb + h * p.lse_sh + s;
    const int64_t arow = b * p.a_sb + (int64_t)s * p.a_ss + h * p.a_sh + 4 * c4;
    // The D/4 lanes of a row all read the running LSE here and lane c4 == 0 stores the new one below: a row's lanes sit
    // in ONE wavefront (launch_fwd_w asserts 64 % (D/4) == 0 and launches 256-thread blocks), so every load is issued
    // before the store in program order -- the value is read once, into a register.
    const float lse_old = p.merge_in ? *lse_p : USP_NEG_INF;
    float mx = lse_old;
    float l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      l[j] = j < p.ksplit ? p.ws_lse[j * slot_l + l_idx] : USP_NEG_INF;
      mx = fmaxf(mx, l[j]);
    }
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    float new_lse = USP_NEG_INF;
    if (mx != USP_NEG_INF) {
      float sum = 0.f, w_old = 0.f;
      if (p.merge_in) { w_old = exp2f((lse_old - mx) * kLog2e); sum = w_old; }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        l[j] = exp2f((l[j] - mx) * kLog2e);          // 0 for an empty cut (lse = -inf) and for j >= ksplit
        sum += l[j];
      }
      const float inv = 1.f / sum;
      new_lse = mx + log2f(sum) * kLn2;
      if (p.merge_in) o = *(const f32x4*)(p.acc + arow) * (w_old * inv);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < p.ksplit) o += *(const f32x4*)(p.ws_o + j * slot_o + o_idx) * (l[j] * inv);
    }
    if (c4 == 0) *lse_p = new_lse;
    if (s >= p.final_begin && s < p.final_end) {
      const u32x2 pk = {E::pack2(o[0], o[1]), E::pack2(o[2], o[3])};
      *(u32x2*)(p.out + 2 * (b * p.o_sb + (int64_t)s * p.o_ss + h * p.o_sh + 4 * c4)) = pk;
    } else {
      *(f32x4*)(p.acc + arow) = o;
    }
  }
}

int launch_split_merge(const FwdArgsT<true>& p, int dtype, int D, hipStream_t st) {
  // same stream as the cuts: the partials are complete when this starts
  if (64 % (D / 4) != 0) return USP_EUNSUPPORTED;           // (the D/4 lanes of a row must share a wavefront: D = 64, 128)
  const int64_t work = (int64_t)p.B * p.Sq * p.Hq * (D / 4);
  const int blocks = (int)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096);
  with_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL((split_merge_kernel<decltype(dt)::value>), dim3(blocks), dim3(256), 0, st, p, D);
  });
  return launched();
}

// What usp_flash_fwd_alibi / _dropout / _sink / _doc add to a plain call; nothing set: usp_flash_fwd.  The entry points fill the
// slopes and their stride, dc, sinks and doc as given; flash_fwd_call checks them and fills al.al_diag and dr, the kernels'
// dropout block (dr.t == 0: off).
struct FwdExtras {
  FwdAlibi al{};
  DropoutCall dc{};
  const float* sinks = nullptr;
  FwdDoc doc{};
  FwdSpan span{};                // (usp_flash_fwd_span: with row_hi, a NULL doc.row_lo is all zero)
  BspCall bsp{};                 // (usp_flash_fwd_bsp: the block mask and the workspace of its lists)
  Dropout dr{};
  FwdMaxl mx{};                  // (usp_flash_fwd_maxlogit: the buffer of row maxima and its strides)
  bool any() const { return al.al_slopes || dr.t || sinks || doc.row_lo || span.row_hi || bsp.mask || mx.row_max; }
};

template <int D, int DT, int NWAVES>
static int launch_fwd_w(FwdArgsSC p, const FwdExtras& x, bool causal, hipStream_t st) {
  p.nq = (p.Sq + 32 * NWAVES - 1) / (32 * NWAVES);
  p.n_items = p.B * p.Hq * p.nq * p.ksplit;
  // persistent launch: one workgroup per resident slot (8 waves: 1 per CU, 4 waves: 2 per CU)
  const int grid = persistent_grid(p.n_items, device_cus() * (NWAVES == 8 ? 1 : 2), p.interleave);
  const size_t lds = 2 * 2 * kBN * D * 2 + (p.sched ? 16 : 0);
  const FwdArgsT<true> ps = p;                               // the argument block of the split kernels
  FwdArgsT<false> plain;                                     // the argument block of the plain kernels: FwdParams alone
  static_cast<FwdParams&>(plain) = p;
  if (x.al.al_slopes) {                                      // ALiBi: instantiations of their own (usp_flash_fwd_alibi.hip)
    FwdArgsAL pa;
    static_cast<FwdArgsT<true>&>(pa) = ps;
    static_cast<FwdAlibi&>(pa) = x.al;
    if (int rc = launch_fwd_alibi(pa, D, DT, causal, NWAVES, grid, lds, st)) return rc;
  } else if (x.dr.t) {                                       // dropout: likewise (usp_flash_fwd_dropout.hip)
    FwdArgsDR pd;
    static_cast<FwdArgsT<true>&>(pd) = ps;
    static_cast<Dropout&>(pd) = x.dr;
    if (int rc = launch_fwd_dropout(pd, D, DT, causal, NWAVES, grid, lds, st)) return rc;
  } else if (x.sinks) {                                      // attention sinks: likewise (usp_flash_fwd_sink.hip)
    FwdArgsSK pk;
    static_cast<FwdArgsT<true>&>(pk) = ps;
    pk.sinks = x.sinks;
    if (int rc = launch_fwd_sink(pk, D, DT, causal, NWAVES, grid, lds, st)) return rc;
  } else if (x.mx.row_max) {                                 // max logits: likewise (usp_flash_fwd_maxl.hip)
    FwdArgsMX pm;
    static_cast<FwdArgsT<true>&>(pm) = ps;
    static_cast<FwdMaxl&>(pm) = x.mx;
    if (int rc = launch_fwd_maxl(pm, D, DT, causal, NWAVES, grid, lds, st)) return rc;
  } else if (x.bsp.mask) {                                   // block-sparse mask: likewise (usp_flash_fwd_bsp.hip), 4 waves only
    if constexpr (NWAVES == 4) {                             // (launch_fwd picks 4 waves under the mask: p.nq counts mask row blocks)
      const BlockLists& bl = x.bsp.layout;
      if (int rc = launch_block_lists(x.bsp.mask, x.bsp.sb, x.bsp.sh, x.bsp.sr, x.bsp.lists, bl, p.Sq, p.Sk, causal, 1, st)) return rc;
      FwdArgsBSP pd;
      static_cast<FwdParams&>(pd) = p;
      pd.bsp_lists = x.bsp.lists; pd.bsp_stride = bl.lf;
      if (int rc = launch_fwd_bsp(pd, D, DT, causal, grid, lds, st)) return rc;
    } else {
      return USP_ELAUNCH;                                    // unreachable: no 8-wave block-sparse instantiation exists
    }
  } else if (x.span.row_hi) {                                // span bound: likewise (usp_flash_fwd_span.hip), never causal
    FwdArgsSPAN pd;
    static_cast<FwdParams&>(pd) = p;
    static_cast<FwdDoc&>(pd) = x.doc;
    static_cast<FwdSpan&>(pd) = x.span;
    if (int rc = launch_fwd_span(pd, D, DT, NWAVES, grid, lds, st)) return rc;
  } else if (x.doc.row_lo) {                                 // document mask: likewise (usp_flash_fwd_doc.hip)
    FwdArgsDOC pd;
    static_cast<FwdParams&>(pd) = p;
    static_cast<FwdDoc&>(pd) = x.doc;
    if (int rc = launch_fwd_doc(pd, D, DT, causal, NWAVES, grid, lds, st)) return rc;
  } else
  with_causal(causal, [&](auto c) {
    constexpr bool C = decltype(c)::value;
    if (p.cap_on)
      hipLaunchKernelGGL((flash_fwd_softcap_kernel<D, DT, C, NWAVES>), dim3(grid), dim3(64 * NWAVES), lds, st, p);
    else if (p.win_on)
      hipLaunchKernelGGL((flash_fwd_window_kernel<D, DT, C, NWAVES>), dim3(grid), dim3(64 * NWAVES), lds, st, ps);
    else if (p.ksplit > 1)
      hipLaunchKernelGGL((flash_fwd_kernel<D, DT, C, NWAVES, true>), dim3(grid), dim3(64 * NWAVES), lds, st, ps);
    else
      hipLaunchKernelGGL((flash_fwd_kernel<D, DT, C, NWAVES>), dim3(grid), dim3(64 * NWAVES), lds, st, plain);
  });
  if (launched() != USP_OK) return USP_ELAUNCH;
  if (p.ksplit > 1) {
    static_assert(64 % (D / 4) == 0 && 256 % (D / 4) == 0, "split_merge_kernel: the D/4 lanes of a row must share a wavefront");
    return launch_split_merge(ps, DT, D, st);
  }
  return USP_OK;
}

template <int D, int DT>
static int launch_fwd(const FwdArgsSC& p, const FwdExtras& x, bool causal, hipStream_t st, int force) {
  // Workgroup shape: 8 waves (256 query rows, one workgroup per CU) stage K/V once per 256 rows and win by
  // 3-4 % whenever they can give every CU work; 4 waves (128 rows, two workgroups per CU) are used only
  // when the 8-wave item list is shorter than the CU count, or for short causal sequences (<= 1024 rows:
  // +3...8 %) (measured with persistent workgroups, profiles/).  Per call, `force` (USP_FORCE_ROW64 / USP_FORCE_WAVE32,
  // include/usp_hip.h) picks the family.  `waves` = 4 | 8, or 64: the 4 x 64-row kernel of usp_flash_fwd64.hip.
  // what usp_flash_fwd64.hip serves (plain and K-split launches; its hand-pinned pipeline has no softcap step)
  const bool fwd64_ok = D == 128 && !p.seq_q && !p.win_on && !p.cap_on && !x.any();   // (... and no ALiBi, dropout, sink or document step)
  const int split_kind = p.ksplit > 1 ? USP_KIND_FWD_SPLIT_MERGE : 0;
  int waves = 64;
  if (!(force & USP_FORCE_ROW64)) {
    const int64_t grid8 = (int64_t)p.B * p.Hq * ((p.Sq + 255) / 256) * p.ksplit;
    // short causal sequences: less diagonal waste (dense only: in packed mode twice the items cost more to fetch)
    // beside a transfer (interleave) RCCL's resident workgroups take a few CUs: with ONE 256-row item per CU a lost
    // CU costs a whole extra round, so the 8-wave kernel halves its granularity there (kbench overlap, 8 resident copy
    // workgroups: 256 items 0.695 vs 0.718 ms; from two items per CU on the 256-row shape wins again, profiles/
    // r02_rank_emulation.txt).  That rule predates the 4 x 64 kernel, which beats the 128-row shape at one item per CU too,
    // alone and beside the copies (round 5, same harness, four launches + 3 x 16 MiB on 8 workgroups: 8192 x 16384 rows x
    // keys, 8 heads = 256 items 1.985 vs 2.081 ms; 8192 x 49152: 5.413 vs 5.773 ms; profiles/r05_fwd_small_interleave.txt):
    // where the 4 x 64 kernel serves the launch the rule no longer applies.
    waves = (grid8 < 256 || (p.interleave && grid8 < 512 && !fwd64_ok) || (!p.seq_q && causal && p.Sq <= 1024)) ? 4 : 8;
    // where the 256-row item wins, the one-wave-per-SIMD kernel (4 waves x 64 rows, usp_flash_fwd64.hip) serves it.  Cut
    // launches: a 64-row item costs more to open and close (64 Q fragments parked, 128 accumulators written as partials),
    // which pays from ~96 tiles per cut on (kbench ksplit, 8-wave split -> 4 x 64 split, merge launch included, round 5:
    // S = 65536 1 head n = 2 1174 -> 1216 TFLOP/s, 32768 2 heads n = 2 1136 -> 1162 and n = 3 1051 -> 1064, 16384 4 heads
    // n = 2 1049 -> 1057; below: 16384 4 heads n = 3 963 -> 945, n = 4 984 -> 957, 8192 6 heads n = 2 799 -> 780;
    // profiles/r05_fwd64_ksplit.txt)
    const bool long_cuts = p.ksplit <= 1 || (int64_t)p.Sk >= (int64_t)96 * kBN * p.ksplit;
    if (waves == 8 && fwd64_ok && long_cuts && !(force & USP_FORCE_WAVE32)) waves = 64;
    if (x.bsp.mask) waves = 4;                               // a block-sparse item is one 128-row mask block
  }
  if (waves == 64) {
    int rc = USP_ELAUNCH;
    if (fwd64_ok && launch_fwd64(p, DT, causal, st, &rc)) {
      if (rc == USP_OK) launch_kinds_note(USP_KIND_FWD_ROW64 | split_kind);
      return rc;
    }
    if (force & USP_FORCE_ROW64) return USP_EUNSUPPORTED;
    waves = 8;                                               // (a layout the 64-row kernel declines)
  }
  const int rc = waves == 4 ? launch_fwd_w<D, DT, 4>(p, x, causal, st) : launch_fwd_w<D, DT, 8>(p, x, causal, st);
  if (rc == USP_OK) launch_kinds_note((waves == 4 ? USP_KIND_FWD_WAVE4 : USP_KIND_FWD_WAVE8) | split_kind);
  return rc;
}

}  // namespace usp

extern "C" int64_t usp_flash_fwd_workspace_bytes(const usp_fwd_args* a, int32_t k_splits) {
  if (!a || k_splits <= 1 || k_splits > 8 || a->seq_q || a->seq_k) return 0;
  const int64_t rows = (int64_t)a->B * a->Sq * a->Hq;
  return (int64_t)k_splits * (rows * a->D + rows) * 4;         // partial outputs + partial LSEs, fp32 (a->D % 4 == 0)
}

// usp_flash_fwd (alibi_slopes == NULL, p_drop == 0, sinks == NULL, row_lo == NULL), usp_flash_fwd_alibi, usp_flash_fwd_dropout,
// usp_flash_fwd_sink, usp_flash_fwd_maxlogit, usp_flash_fwd_doc and usp_flash_fwd_span
static int flash_fwd_call(const usp_fwd_args* a, usp::FwdExtras x, void* stream) {
  using namespace usp;
  launch_kinds_reset();
  if (!a || !a->lse) return USP_EINVAL;
  if (int rc = check_force(a->flags)) return rc;
  if (int rc = check_problem(*a)) return rc;
  if (int rc = check_alibi(*a, x.al.al_slopes, x.al.al_sb)) return rc;
  if (int rc = check_dropout(*a, x.dc, &x.dr)) return rc;
  if (int rc = check_sink(*a, x.sinks)) return rc;
  if (int rc = check_maxl(*a, x.mx.row_max, x.mx.row_max_sb, x.mx.row_max_sh)) return rc;
  // (with row_hi the span's check judges every stride before any decline; it declines all the document's check does)
  if (int rc = check_doc(*a, x.doc.row_lo != nullptr && !x.span.row_hi, x.doc.row_lo_sb, 0)) return rc;
  if (int rc = check_span(*a, x.span.row_hi != nullptr, x.doc.row_lo_sb, x.span.row_hi_sb, 0, 0)) return rc;
  if (int rc = check_bsp(*a, x.bsp.mask, x.bsp.sb, x.bsp.sh, x.bsp.sr, x.bsp.lists)) return rc;
  if (x.bsp.mask) x.bsp.layout = block_lists(a->B, a->Hq, (a->Sq + 127) / 128, (a->Sk + 127) / 128);   // once per call
  if (!tensor_aligned(a->q, 16, 8) || !tensor_aligned(a->k, 16, 8) || !tensor_aligned(a->v, 16, 8))
    return USP_EUNSUPPORTED;
  const bool packed = a->seq_q != nullptr || a->seq_k != nullptr;
  if (packed && !(a->seq_q && a->seq_k)) return USP_EINVAL;
  const Mask mask = decode_mask(*a);
  if (packed && (mask.windowed || mask.shifted)) return USP_EUNSUPPORTED;        // dense launches only
  const int f_all = packed ? 2 : a->Sq;          // packed: final_begin/_end count half sequences (0,1,2)
  int fb = a->final_begin < 0 ? 0 : a->final_begin;
  int fe = a->final_end > f_all ? f_all : a->final_end;
  if (fe < fb) fe = fb;
  const bool any_final = fe > fb, any_acc = (fb > 0 || fe < f_all);
  if (any_final && !tensor_aligned(a->out, 8, 4)) return a->out.ptr ? USP_EUNSUPPORTED : USP_EINVAL;
  if ((any_acc || a->merge_in) && !tensor_aligned(a->acc, 16, 4)) return a->acc.ptr ? USP_EUNSUPPORTED : USP_EINVAL;

  FwdArgsSC p;
  p.q = (const char*)a->q.ptr; p.k = (const char*)a->k.ptr; p.v = (const char*)a->v.ptr;
  p.out = (char*)a->out.ptr; p.acc = (float*)a->acc.ptr; p.lse = a->lse;
  p.q_sb = a->q.stride_b; p.q_ss = a->q.stride_s; p.q_sh = a->q.stride_h;
  p.k_sb = a->k.stride_b; p.k_ss = a->k.stride_s; p.k_sh = a->k.stride_h;
  p.v_sb = a->v.stride_b; p.v_ss = a->v.stride_s; p.v_sh = a->v.stride_h;
  p.o_sb = a->out.stride_b; p.o_ss = a->out.stride_s; p.o_sh = a->out.stride_h;
  p.a_sb = a->acc.stride_b; p.a_ss = a->acc.stride_s; p.a_sh = a->acc.stride_h;
  p.lse_sb = a->lse_stride_b; p.lse_sh = a->lse_stride_h;
  p.B = a->B; p.Sq = a->Sq; p.Sk = a->Sk; p.Hq = a->Hq; p.Hkv = a->Hkv;
  p.G = a->Hq / a->Hkv;
  p.nq = 0;   // set per workgroup shape in launch_fwd_w
  mask.store(p);
  p.scale = a->softmax_scale;
  p.scale_log2 = a->softmax_scale * kLog2e;
  p.merge_in = a->merge_in ? 1 : 0;
  p.final_begin = fb; p.final_end = fe;
  p.out_wide = tensor_aligned(a->out, 16, 8) ? 1 : 0;
  p.seq_q = a->seq_q; p.seq_k = a->seq_k;
  p.sched = packed ? a->sched : nullptr;
  p.interleave = (a->flags & USP_LAUNCH_INTERLEAVE) ? 1 : 0;
  p.walk_g = p.G;                                  // a KV group's heads side by side in the item walk
  p.ksplit = 1; p.ws_o = nullptr; p.ws_lse = nullptr;
  if (a->k_splits > 1 && a->workspace != nullptr && !x.doc.row_lo && !x.span.row_hi && !x.bsp.mask && !x.mx.row_max) {   // (a document, span, block-sparse or max-logit launch is served uncut: usp_hip.h)
    if (packed) return USP_EUNSUPPORTED;                       // dense launches only
    if (a->k_splits > 8 || !aligned(a->workspace, 16)) return USP_EINVAL;
    if ((any_acc || a->merge_in) && (a->acc.stride_h % 4 != 0)) return USP_EUNSUPPORTED;
    p.ksplit = a->k_splits;
    p.ws_o = (float*)a->workspace;
    p.ws_lse = p.ws_o + (int64_t)p.ksplit * a->B * a->Sq * a->Hq * a->D;
  }
  if (packed) p.q_sb = p.k_sb = p.v_sb = p.o_sb = p.a_sb = p.lse_sb = 0;
  x.al.al_diag = alibi_diag(*a);
  const int force = a->flags & (USP_FORCE_ROW64 | USP_FORCE_WAVE32);
  return with_head_dim_dtype(a->D, a->dtype, [&](auto d, auto dt) {
    return launch_fwd<decltype(d)::value, decltype(dt)::value>(p, x, mask.causal, (hipStream_t)stream, force);
  });
}

extern "C" int usp_flash_fwd(const usp_fwd_args* a, void* stream) { return flash_fwd_call(a, usp::FwdExtras{}, stream); }

extern "C" int usp_flash_fwd_alibi(const usp_fwd_args* a, const float* alibi_slopes, int64_t alibi_stride_b, void* stream) {
  usp::FwdExtras x;
  x.al.al_slopes = alibi_slopes; x.al.al_sb = alibi_stride_b;
  return flash_fwd_call(a, x, stream);
}

extern "C" int usp_flash_fwd_dropout(const usp_fwd_args* a, float p_drop, uint64_t seed, int32_t row0, int32_t key0, int32_t head0,
                                     void* stream) {
  usp::FwdExtras x;
  x.dc = usp::DropoutCall{p_drop, seed, row0, key0, head0};
  return flash_fwd_call(a, x, stream);
}

extern "C" int usp_flash_fwd_sink(const usp_fwd_args* a, const float* sinks, void* stream) {
  usp::FwdExtras x;
  x.sinks = sinks;
  return flash_fwd_call(a, x, stream);
}

extern "C" int usp_flash_fwd_maxlogit(const usp_fwd_args* a, float* row_max, int64_t row_max_stride_b, int64_t row_max_stride_h,
                                       void* stream) {
  usp::FwdExtras x;                                                   // row_max == NULL: exactly usp_flash_fwd
  if (row_max) x.mx = usp::FwdMaxl{row_max, row_max_stride_b, row_max_stride_h};
  return flash_fwd_call(a, x, stream);
}

extern "C" int usp_flash_fwd_doc(const usp_fwd_args* a, const int32_t* row_lo, int64_t row_lo_stride_b, void* stream) {
  usp::FwdExtras x;
  x.doc = usp::FwdDoc{row_lo, row_lo ? row_lo_stride_b : 0};
  return flash_fwd_call(a, x, stream);
}

extern "C" int usp_flash_fwd_span(const usp_fwd_args* a, const int32_t* row_lo, int64_t row_lo_stride_b, const int32_t* row_hi,
                                  int64_t row_hi_stride_b, void* stream) {
  usp::FwdExtras x;
  x.doc = usp::FwdDoc{row_lo, row_lo ? row_lo_stride_b : 0};         // row_hi == NULL: exactly usp_flash_fwd_doc
  x.span = usp::FwdSpan{row_hi, row_hi ? row_hi_stride_b : 0};
  return flash_fwd_call(a, x, stream);
}

extern "C" int usp_flash_fwd_bsp(const usp_fwd_args* a, const void* mask, int64_t mask_stride_b, int64_t mask_stride_h,
                                 int64_t mask_stride_row, void* lists, void* stream) {
  usp::FwdExtras x;                                                   // mask == NULL: exactly usp_flash_fwd
  if (mask) x.bsp = usp::BspCall{mask, mask_stride_b, mask_stride_h, mask_stride_row, (int*)lists};
  return flash_fwd_call(a, x, stream);
}
