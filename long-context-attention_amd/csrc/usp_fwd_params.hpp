// Argument blocks and LDS-layout constants shared by the forward kernels (usp_flash_fwd.hip: 8 / 4 waves x 32 query
// rows, two waves per SIMD; usp_flash_fwd64.hip: 4 waves x 64 query rows, one wave per SIMD).
#pragma once
#include "usp_common.hpp"
#include "usp_dropout_rng.h"

namespace usp {

struct FwdParams {
  const char* q; const char* k; const char* v;
  char* out; float* acc; float* lse;
  int64_t q_sb, q_ss, q_sh;
  int64_t k_sb, k_ss, k_sh;
  int64_t v_sb, v_ss, v_sh;
  int64_t o_sb, o_ss, o_sh;
  int64_t a_sb, a_ss, a_sh;
  int64_t lse_sb, lse_sh;
  int B, Sq, Sk, Hq, Hkv, G, nq, n_items;
  int causal_off;                 // Sk - Sq
  float scale, scale_log2;
  int merge_in, final_begin, final_end;
  int out_wide;                   // out rows are 16-byte aligned: 16-byte epilogue stores
  const int* seq_q; const int* seq_k;   // packed variable-length batch: B (first row, rows) pairs, or NULL
  int* sched;                           // packed mode: control block of the dynamic item queue, or NULL
  int interleave;                       // USP_LAUNCH_INTERLEAVE: one workgroup per item (collectives can slip in)
  int walk_g;                           // 64-row kernel: query heads of a KV group walked side by side (usp_item_deal.h: usp_group_item); 1 = off
};

// K split (dense mode): every (batch, head, query tile) is cut into `ksplit` items along K; partial results go to
// [ksplit][B,Sq,Hq,D] fp32 and [ksplit][B,Hq,Sq] fp32.  Kernel arguments of the split instantiation ONLY: the plain
// kernels keep the argument block (and with it the machine code) they were profiled with.
struct FwdSplit {
  int ksplit;
  float* ws_o; float* ws_lse;
  // Sliding window, left bound (ABI v5): query row i sees key j only if j >= i + win_lo (win_lo = Sk - Sq - window_left).
  // Lives in the split instantiation: tiles left of a query tile's window are skipped by the same rebasing the K split
  // uses, and every tile of a windowed launch takes the generic (masked) loop.  The RIGHT bound needs nothing new: it
  // is the causal limit with a shifted offset (host: causal_off = Sk - Sq + window_right, causal instantiation).
  int win_on, win_lo;
};
template <bool KS> struct FwdArgsT : FwdParams {};
template <> struct FwdArgsT<true> : FwdParams, FwdSplit {};
// Logit soft-capping (USP_ATTN_SOFTCAP): kernel arguments of the softcap instantiations only (flash_fwd_softcap_kernel, built on
// the split instantiation's generic loop); the plain and split kernels keep their argument blocks and machine code.
struct FwdSoftcap {
  int cap_on;                           // host: the call caps its scores (selects the softcap kernel)
  float cap_log2;                       // cap * log2(e): the capped score in exp2 units is cap_log2 * tanh(..)
  float tanh_k2;                        // 2 * scale * log2(e) / cap (usp_common.hpp: softcap_tanh)
};
struct FwdArgsSC : FwdArgsT<true>, FwdSoftcap {};
// ALiBi (usp_flash_fwd_alibi): kernel arguments of the ALiBi instantiations only (usp_flash_fwd_alibi.hip:
// flash_fwd_alibi_kernel, built on the split instantiation's generic loop like the softcap kernels); every other kernel keeps
// its argument block and machine code.
struct FwdAlibi {
  const float* al_slopes;               // fp32 slopes: head h of batch b at al_slopes[b * al_sb + h]; NULL = no ALiBi
  int64_t al_sb;                        // batch stride in elements (0: one (Hq,) vector for the whole batch)
  int al_diag;                          // Sk - Sq + mask_shift: the bias of (row i, key j) is -slope * |i + al_diag - j|.  A field
                                        // of its own: causal_off also absorbs window_right and is dropped with a bound that cuts nothing
};
struct FwdArgsAL : FwdArgsT<true>, FwdAlibi {};
// Dropout (usp_flash_fwd_dropout): kernel arguments of the dropout instantiations only (usp_flash_fwd_dropout.hip:
// flash_fwd_dropout_kernel, built on the split instantiation's generic loop like the softcap and ALiBi kernels); every other
// kernel keeps its argument block and machine code.  The mask and the `Dropout` block are csrc/usp_dropout_rng.h.
struct FwdArgsDR : FwdArgsT<true>, Dropout {};
// Attention sinks (usp_flash_fwd_sink): kernel arguments of the sink instantiations only (usp_flash_fwd_sink.hip:
// flash_fwd_sink_kernel, the split and window instantiations' tile loops with the sink merged in the epilogue); every other
// kernel keeps its argument block and machine code.
struct FwdSink {
  const float* sinks;                   // fp32 (Hq,): the sink logit of query head h, in score units (not scaled)
};
struct FwdArgsSK : FwdArgsT<true>, FwdSink {};
struct FwdArgsSKP : FwdArgsT<false>, FwdSink {};      // ... of the sink kernels on the plain (unsplit) argument block
// Document mask (usp_flash_fwd_doc): kernel arguments of the document instantiations only (usp_flash_fwd_doc.hip:
// flash_fwd_doc_kernel, the plain kernel's loops under the window kernel's rotated walk); every other kernel keeps its
// argument block and machine code.
struct FwdDoc {
  const int* row_lo;                    // int32 (Sq,): the first key row i sees, in the launch's key numbering; NULL = no bound
  int64_t row_lo_sb;                    // batch stride in elements (0: one array for the whole batch)
};
struct FwdArgsDOC : FwdArgsT<false>, FwdDoc {};
// Span bound (usp_flash_fwd_span): kernel arguments of the span instantiations only (usp_flash_fwd_span.hip: flash_fwd_span_kernel,
// the document kernel with a right key bound read per row in place of the causal diagonal); every other kernel keeps its
// argument block and machine code.
struct FwdSpan {
  const int* row_hi;                    // int32 (Sq,): one past the last key row i sees, in the launch's key numbering; NULL = no span launch
  int64_t row_hi_sb;                    // batch stride in elements (0: one array for the whole batch)
};
struct FwdArgsSPAN : FwdArgsT<false>, FwdDoc, FwdSpan {};      // (row_lo may be NULL here: all zero)
// Block-sparse mask (usp_flash_fwd_bsp): kernel arguments of the block-sparse instantiations only (usp_flash_fwd_bsp.hip:
// flash_fwd_bsp_kernel, the plain kernel's loops walking a list of key tiles); every other kernel keeps its argument block and
// machine code.  The lists are built by usp_block_lists.hip (layout: BlockLists below).
struct FwdBsp {
  const int* bsp_lists;                 // int32: the list of item (b, h, 128-row block r) starts at ((b * Hq + h) * nq + r) * bsp_stride
  int bsp_stride;                       // ints per list: [0] = count, [1 ..] = ascending 64-key tile indices
};
struct FwdArgsBSP : FwdArgsT<false>, FwdBsp {};
// Max logits (usp_flash_fwd_maxlogit): kernel arguments of the max-logit instantiations only (usp_flash_fwd_maxl.hip:
// flash_fwd_maxl_kernel, the plain and window kernels' tile loops with a true row maximum kept beside the lazy reference); every
// other kernel keeps its argument block and machine code.
struct FwdMaxl {
  float* row_max;                       // fp32 (B, Hq, Sq), seq stride 1: max over the keys row i sees of softmax_scale * q_i . k_j
  int64_t row_max_sb, row_max_sh;       // batch and head strides in elements
};
struct FwdArgsMX : FwdArgsT<true>, FwdMaxl {};
struct FwdArgsMXP : FwdArgsT<false>, FwdMaxl {};      // ... of the max-logit kernels on the plain (unsplit) argument block

constexpr int kBN = 64;    // keys per KV tile

template <int D> struct KSwz {
  // 16-byte slots per K row and rows per 256-byte LDS bank row
  static constexpr int SPR = D / 8;
  static constexpr int RPB = 16 / SPR < 1 ? 1 : 16 / SPR;
  static USP_DEV int of(int row) { return (row / RPB) & (SPR - 1); }
};

// The 64-rows-per-wave forward (usp_flash_fwd64.hip): dense launches of D = 128, plain or K-split (no window, no packed
// batch).  Returns false when the launch is not one it serves (the caller then takes the 8-wave kernel).
bool launch_fwd64(const FwdArgsT<true>& p, int dtype, bool causal, hipStream_t st, int* rc);
// The merge launch behind a K-split forward (usp_flash_fwd.hip: split_merge_kernel), same stream.
int launch_split_merge(const FwdArgsT<true>& p, int dtype, int D, hipStream_t st);
// The ALiBi forward (usp_flash_fwd_alibi.hip): flash_fwd_alibi_kernel<D, dtype, causal, waves> (waves = 4 | 8) on `grid`
// workgroups with `lds` bytes; `p` is complete (nq / n_items included).  Returns USP_OK / USP_ELAUNCH / USP_EUNSUPPORTED.
int launch_fwd_alibi(const FwdArgsAL& p, int D, int dtype, bool causal, int waves, int grid, size_t lds, hipStream_t st);
// The dropout forward (usp_flash_fwd_dropout.hip), likewise.
int launch_fwd_dropout(const FwdArgsDR& p, int D, int dtype, bool causal, int waves, int grid, size_t lds, hipStream_t st);
// The sink forward (usp_flash_fwd_sink.hip), likewise; p.win_on picks the window form, p.ksplit > 1 the split form, else the plain one.
int launch_fwd_sink(const FwdArgsSK& p, int D, int dtype, bool causal, int waves, int grid, size_t lds, hipStream_t st);
// The document-mask forward (usp_flash_fwd_doc.hip), likewise; `lds` is the plain kernel's, the launch adds the bounds' room.
int launch_fwd_doc(const FwdArgsDOC& p, int D, int dtype, bool causal, int waves, int grid, size_t lds, hipStream_t st);
// The span forward (usp_flash_fwd_span.hip), likewise; never causal: the diagonal is folded into row_hi.
int launch_fwd_span(const FwdArgsSPAN& p, int D, int dtype, int waves, int grid, size_t lds, hipStream_t st);
// The block-sparse forward (usp_flash_fwd_bsp.hip), likewise; always the 4-wave shape: one work item is one 128-row mask block.
int launch_fwd_bsp(const FwdArgsBSP& p, int D, int dtype, bool causal, int grid, size_t lds, hipStream_t st);
// The max-logit forward (usp_flash_fwd_maxl.hip), likewise; p.win_on picks the window form, else the plain one (p.ksplit is 1).
int launch_fwd_maxl(const FwdArgsMX& p, int D, int dtype, bool causal, int waves, int grid, size_t lds, hipStream_t st);

}  // namespace usp
