// Host side of libusp_hip.so: what sits between the C ABI (include/usp_hip.h) and the kernel launches, once.
// Everything here is host code (it names HIP runtime calls); nothing in it is reachable from a __device__ path.
// A call's behaviour comes from its argument block alone: the library reads no environment.
#pragma once
#include <atomic>
#include <type_traits>

#include "usp_common.hpp"
#include "usp_hip.h"
#include "usp_dropout_rng.h"
#include "usp_mask_decode.h"

namespace usp {

// Record which kernels a flash call launches (usp_last_launch_kinds; defined in usp_elementwise.hip)
void launch_kinds_reset();
void launch_kinds_note(int kind);

// Result of the launch just issued on this thread.
inline int launched() { return hipGetLastError() == hipSuccess ? USP_OK : USP_ELAUNCH; }

// Compute units of the CURRENT device, asked once per device id (two threads asking at once both get the answer and store
// the same value); 256 where there is no device.
inline int device_cus() {
  constexpr int kMaxDevices = 64;
  static std::atomic<int> cached[kMaxDevices];     // 0 = not asked yet
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  const bool slot = dev >= 0 && dev < kMaxDevices;
  if (slot && (n = cached[dev].load(std::memory_order_relaxed)) > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  if (slot) cached[dev].store(n, std::memory_order_relaxed);
  return n;
}

// Persistent launch: one workgroup per resident slot, each walking a list of items; USP_LAUNCH_INTERLEAVE, or fewer items
// than slots: one workgroup per item (the same kernel: its list then has one entry).
inline int persistent_grid(int n_items, int slots, int interleave) {
  return (!interleave && n_items > slots) ? slots : n_items;
}

// ---- alignment: base pointer on a `bytes` boundary, every stride a multiple of `elems` elements ----
inline bool aligned(const void* ptr, int bytes) { return (reinterpret_cast<uintptr_t>(ptr) & (uintptr_t)(bytes - 1)) == 0; }
inline bool tensor_aligned(const void* ptr, int64_t sb, int64_t ss, int64_t sh, int bytes, int elems) {
  return ptr && aligned(ptr, bytes) && sb % elems == 0 && ss % elems == 0 && sh % elems == 0;
}
inline bool tensor_aligned(const usp_tensor& t, int bytes, int elems) {
  return tensor_aligned(t.ptr, t.stride_b, t.stride_s, t.stride_h, bytes, elems);
}

// ---- what the 64-row kernels' LDS-DMA asks of a streamed tensor's row stride (`stride_s`, in 16-bit elements): per-lane
// offsets and the pieces' scalar offsets are 32-bit, so 64 rows span less than 2^31 bytes; where the pieces' slot swizzle is
// XORed into the per-lane byte offset (`swizzled`), the row pitch is a multiple of 256 bytes ----
inline bool dma_rows_ok(int64_t stride_s, bool swizzled) {
  return stride_s * 128 < (1LL << 31) && (!swizzled || (stride_s * 2) % 256 == 0);
}

// ---- run-time (dtype, causal, head dim) -> template arguments: f receives std::integral_constants ----
template <int V> using Int = std::integral_constant<int, V>;
template <class F> auto with_dtype(int dtype, F&& f) { return dtype == USP_BF16 ? f(Int<0>{}) : f(Int<1>{}); }
template <class F> auto with_causal(bool causal, F&& f) { return causal ? f(std::true_type{}) : f(std::false_type{}); }
template <class F> auto with_dtype_causal(int dtype, bool causal, F&& f) {
  return with_dtype(dtype, [&](auto dt) { return with_causal(causal, [&](auto c) { return f(dt, c); }); });
}
// f(Int<D>, Int<DT>) -> int; USP_EUNSUPPORTED for a head dim without kernels
template <class F> int with_head_dim_dtype(int D, int dtype, F&& f) {
  return with_dtype(dtype, [&](auto dt) -> int {
    switch (D) {
      case 32: return f(Int<32>{}, dt);
      case 64: return f(Int<64>{}, dt);
      case 128: return f(Int<128>{}, dt);
    }
    return USP_EUNSUPPORTED;
  });
}

// ---- what usp_flash_fwd and usp_flash_bwd check alike (Args = usp_fwd_args / usp_bwd_args), in the order they check it ----
inline int check_force(int flags) {
  return (flags & USP_FORCE_ROW64) && (flags & USP_FORCE_WAVE32) ? USP_EINVAL : USP_OK;
}
template <class Args> int check_problem(const Args& a) {
  if (a.dtype != USP_BF16 && a.dtype != USP_FP16) return USP_EINVAL;
  if (a.B <= 0 || a.Sq <= 0 || a.Sk <= 0 || a.Hq <= 0 || a.Hkv <= 0) return USP_EINVAL;
  if (!(a.softmax_scale > 0.f)) return USP_EINVAL;
  const bool has_cap = (a.flags & USP_ATTN_SOFTCAP) != 0;     // (the field is read only with the bit)
  if (has_cap && !(__builtin_isfinite(a.softcap) && a.softcap > 0.f)) return USP_EINVAL;
  if (has_cap && (a.flags & USP_FORCE_ROW64)) return USP_EUNSUPPORTED;   // the 64-row family declines softcap
  if ((a.flags & USP_ATTN_SHIFT) && (a.mask_shift >= (1 << 30) || a.mask_shift <= -(1 << 30))) return USP_EINVAL;
  if (a.D != 32 && a.D != 64 && a.D != 128) return USP_EUNSUPPORTED;
  if (a.Hq % a.Hkv != 0) return USP_EUNSUPPORTED;
  return USP_OK;
}

// What every extra of a call -- ALiBi, dropout, sinks, the document mask: the entry points beside usp_flash_fwd / usp_flash_bwd --
// declines alike.  The checks below run in the order alibi, dropout, sink, doc, each with its own USP_EINVAL cases and declines
// first and this last, before anything is launched or written.
template <class Args> int check_extras(const Args& a) {
  if (a.flags & USP_ATTN_SOFTCAP) return USP_EUNSUPPORTED;          // no instantiation holds both steps
  if (a.seq_q || a.seq_k) return USP_EUNSUPPORTED;                  // dense launches only
  if (a.flags & USP_FORCE_ROW64) return USP_EUNSUPPORTED;           // the 64-row family declines them
  return USP_OK;
}

// ALiBi (usp_flash_fwd_alibi / usp_flash_bwd_alibi).  NULL slopes: the call is usp_flash_fwd / usp_flash_bwd, whatever the stride.
template <class Args> int check_alibi(const Args& a, const float* slopes, int64_t stride_b) {
  if (!slopes) return USP_OK;
  if (stride_b < 0) return USP_EINVAL;
  return check_extras(a);
}
// The bias diagonal: the bias of (row i, key j) is -slope * |i + diag - j|, diag = Sk - Sq + mask_shift.  Not taken from the
// decoded mask: causal_off also absorbs window_right, and a bound that cuts nothing is dropped there -- the bias is not.
// |mask_shift| < 2^30 (check_problem) and Sq + Sk < 2^29 keep it in int.
template <class Args> int alibi_diag(const Args& a) {
  return (int)((int64_t)a.Sk - a.Sq + ((a.flags & USP_ATTN_SHIFT) ? a.mask_shift : 0));
}

// Dropout (usp_flash_fwd_dropout / usp_flash_bwd_dropout): validates the scalars and fills the kernels' block.  p_drop == 0, or one
// whose keep threshold is 256, leaves dr->t = 0: the call is usp_flash_fwd / usp_flash_bwd and the offsets are not looked at.
// What usp_flash_fwd_dropout / usp_flash_bwd_dropout add to a call (p_drop = 0: nothing)
struct DropoutCall { float p_drop; uint64_t seed; int32_t row0, key0, head0; };

template <class Args>
int check_dropout(const Args& a, const DropoutCall& dc, Dropout* dr) {
  const float p_drop = dc.p_drop;
  const uint64_t seed = dc.seed;
  const int32_t row0 = dc.row0, key0 = dc.key0, head0 = dc.head0;
  *dr = Dropout{};
  if (!(p_drop >= 0.f) || !(p_drop < 1.f)) return USP_EINVAL;       // NaN, negative, >= 1
  const int t = usp_dropout_threshold(p_drop);
  if (p_drop == 0.f || t >= 256) return USP_OK;
  if (row0 < 0 || key0 < 0 || head0 < 0) return USP_EINVAL;
  if ((row0 & 3) || (key0 & 3)) return USP_EUNSUPPORTED;             // a DPP quad of lanes shares one 4 x 4 patch
  if ((int64_t)row0 + a.Sq >= (1LL << 31) || (int64_t)key0 + a.Sk >= (1LL << 31)) return USP_EUNSUPPORTED;
  if (int rc = check_extras(a)) return rc;
  dr->k0 = (uint32_t)(seed & 0xffffffffu);
  dr->k1 = (uint32_t)(seed >> 32);
  dr->row0 = (uint32_t)row0; dr->key0 = (uint32_t)key0; dr->head0 = (uint32_t)head0;
  dr->t = (uint32_t)t;
  dr->rs = 256.f / (float)t;
  dr->irs = (float)t / 256.f;
  return USP_OK;
}

// Attention sinks (usp_flash_fwd_sink).  NULL sinks: the call is usp_flash_fwd.
inline int check_sink(const usp_fwd_args& a, const float* sinks) {
  if (!sinks) return USP_OK;
  if (a.merge_in) return USP_EINVAL;                                // the sink belongs to the launch that opens the rows' state
  return check_extras(a);
}

// Max logits (usp_flash_fwd_maxlogit).  NULL row_max: the call is usp_flash_fwd, whatever the strides.
inline int check_maxl(const usp_fwd_args& a, const float* row_max, int64_t stride_b, int64_t stride_h) {
  if (!row_max) return USP_OK;
  if (stride_b < 0 || stride_h < 0 || !aligned(row_max, 4)) return USP_EINVAL;
  return check_extras(a);
}

// Document mask (usp_flash_fwd_doc / usp_flash_bwd_doc).  No array: the call is usp_flash_fwd / usp_flash_bwd, whatever the strides.
template <class Args> int check_doc(const Args& a, bool has_doc, int64_t row_lo_stride_b, int64_t key_hi_stride_b) {
  if (!has_doc) return USP_OK;
  if (row_lo_stride_b < 0 || key_hi_stride_b < 0) return USP_EINVAL;
  if (a.flags & (USP_ATTN_WINDOW | USP_ATTN_SHIFT)) return USP_EUNSUPPORTED;   // no second bound beside it
  return check_extras(a);
}

// Span bound (usp_flash_fwd_span / usp_flash_bwd_span).  No row_hi / key_lo: the call is usp_flash_fwd_doc / usp_flash_bwd_doc on the
// remaining arrays.  With them the diagonal lies in the arrays: a causal call is declined, and the rest is the document's list.
template <class Args> int check_span(const Args& a, bool has_span, int64_t stride_a, int64_t stride_b, int64_t stride_c, int64_t stride_d) {
  if (!has_span) return USP_OK;
  if (stride_a < 0 || stride_b < 0 || stride_c < 0 || stride_d < 0) return USP_EINVAL;
  if (a.causal) return USP_EUNSUPPORTED;                            // the planner folds the diagonal into row_hi
  if (a.flags & (USP_ATTN_WINDOW | USP_ATTN_SHIFT)) return USP_EUNSUPPORTED;   // no third bound beside them
  return check_extras(a);
}

// Block-sparse mask (usp_flash_fwd_bsp / usp_flash_bwd_bsp).  NULL mask: the call is usp_flash_fwd / usp_flash_bwd, whatever the rest.
template <class Args> int check_bsp(const Args& a, const void* mask, int64_t stride_b, int64_t stride_h, int64_t stride_row, const void* lists) {
  if (!mask) return USP_OK;
  if (stride_b < 0 || stride_h < 0 || stride_row < 0) return USP_EINVAL;
  if (!lists || !aligned(lists, 4)) return USP_EINVAL;
  if (a.flags & (USP_ATTN_WINDOW | USP_ATTN_SHIFT)) return USP_EUNSUPPORTED;   // no bound beside the mask
  if (a.Sq != a.Sk) return USP_EUNSUPPORTED;                        // whole blocks of one sequence against itself
  return check_extras(a);
}
// The lists of a block-sparse call in the caller's workspace (usp_block_lists.hip builds them, the kernels of usp_flash_fwd_bsp.hip /
// usp_flash_bwd_bsp.hip read them), in ints: bh * nrb forward lists of `lf` ints, then from off_q bh * nqb dQ lists of `lf` ints (nqb
// pairs of row blocks), then from off_t bh * nkb transposed lists of `lt` ints; every list is [count, entries ...].
struct BlockLists {
  int64_t bh;                   // B * Hq
  int hq, nrb, nqb, nkb;
  int lf, lt;
  int64_t off_q, off_t, ints;
};
inline BlockLists block_lists(int B, int Hq, int nrb, int nkb) {
  BlockLists l;
  l.bh = (int64_t)B * Hq; l.hq = Hq; l.nrb = nrb; l.nqb = (nrb + 1) / 2; l.nkb = nkb;
  l.lf = 2 * nkb + 2; l.lt = 2 * nrb + 2;
  l.off_q = l.bh * nrb * l.lf;
  l.off_t = l.off_q + l.bh * l.nqb * l.lf;
  l.ints = l.off_t + l.bh * nkb * l.lt;
  return l;
}
// What usp_flash_fwd_bsp / usp_flash_bwd_bsp add to a plain call (mask == NULL: nothing)
struct BspCall {
  const void* mask = nullptr;
  int64_t sb = 0, sh = 0, sr = 0;
  int* lists = nullptr;
  BlockLists layout{};          // of `lists`, computed once per call (flash_fwd_call / flash_bwd_call) and handed down
};
// The builder launch (usp_block_lists.hip); which: bit 0 = forward lists, bit 1 = dQ lists, bit 2 = transposed (dK/dV) lists
int launch_block_lists(const void* mask, int64_t sb, int64_t sh, int64_t sr, int* ws, const BlockLists& l, int Sq, int Sk, bool causal,
                       int which, hipStream_t st);

// Sliding window (flash-attn's window_size) and softcap of a call, as the kernels take them: causal caps the right bound
// at 0; a right bound is the causal limit with a shifted offset (causal instantiation); a left bound is a second mask term
// (forward: the split instantiation, FwdSplit).
struct Mask {
  bool causal;                  // the causal instantiation runs: a.causal or a right window bound -- where it cuts a (row, key) pair
  bool shifted;                 // USP_ATTN_SHIFT is set: dense launches only
  bool windowed;                // a bound beyond plain causal: dense launches only
  int causal_off, win_on, win_lo, cap_on;
  float cap_log2, tanh_k2;
  template <class Params> void store(Params& p) const {
    p.causal_off = causal_off; p.win_on = win_on; p.win_lo = win_lo;
    p.cap_on = cap_on; p.cap_log2 = cap_log2; p.tanh_k2 = tanh_k2;
  }
};
template <class Args> Mask decode_mask(const Args& a) {
  const bool has_win = (a.flags & USP_ATTN_WINDOW) != 0, has_cap = (a.flags & USP_ATTN_SOFTCAP) != 0;
  // USP_ATTN_SHIFT moves the diagonal both bounds hang on, and nothing else: to the kernels it is another causal_off / win_lo.
  // The integer part (64-bit sums; a bound that cuts nothing dropped, one that cuts everything saturated) is plain C and
  // checked on the host: usp_mask_decode.h.
  const usp_mask_bounds mb = usp_decode_mask_bounds(a.Sq, a.Sk, a.causal ? 1 : 0, has_win ? 1 : 0, has_win ? a.window_left : -1,
                                                    has_win ? a.window_right : -1, (a.flags & USP_ATTN_SHIFT) ? 1 : 0,
                                                    (a.flags & USP_ATTN_SHIFT) ? a.mask_shift : 0);
  Mask m;
  m.causal = mb.causal != 0;
  m.windowed = mb.windowed != 0;
  m.causal_off = mb.causal_off;
  m.win_on = mb.win_on;
  m.win_lo = mb.win_lo;
  m.shifted = (a.flags & USP_ATTN_SHIFT) != 0;
  m.cap_on = has_cap ? 1 : 0;
  m.cap_log2 = has_cap ? a.softcap * kLog2e : 0.f;
  m.tanh_k2 = has_cap ? 2.f * a.softmax_scale * kLog2e / a.softcap : 0.f;
  return m;
}

}  // namespace usp
