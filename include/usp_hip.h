/*
 * usp_hip.h -- C ABI of libusp_hip.so, the MI355X (gfx950) device library behind the
 * Unified-Sequence-Parallel attention path.
 *
 * The reference (feifeibear/long-context-attention, "yunchang" v0.6.4) is pure Python and has no
 * FFI of its own: its device arithmetic lives in third-party ops reached through the selector
 * seam `select_flash_attn_impl` (yunchang/kernels/__init__.py:63-65).  Each entry point below
 * replaces one of those call sites (cited per function); the Python binding a maintainer adds is
 * a ctypes stub, shown in INTEGRATION.md and implemented in long-context-attention_amd/_C.py.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated;
 *   - tensors are (batch, seq, head, dim) with dim contiguous; strides are in ELEMENTS;
 *   - nothing allocates, nothing synchronises, nothing touches any stream but `stream`
 *     (a hipStream_t passed as void*; NULL = the legacy default stream);
 *   - thread-safe and re-entrant: no mutable globals;
 *   - return 0 on success, a negative USP_E* code otherwise (the launch is then not issued);
 *     usp_strerror() maps codes to text.
 */
#ifndef USP_HIP_H
#define USP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define USP_ABI_VERSION 7

enum { USP_BF16 = 0, USP_FP16 = 1 };

enum {
  USP_OK = 0,
  USP_EINVAL = -1,      /* bad argument (null pointer, non-positive size, bad dtype) */
  USP_EUNSUPPORTED = -2,/* head_dim not in {32, 64, 128}, Hq % Hkv != 0, misaligned pointer/stride */
  USP_ELAUNCH = -3      /* hipLaunchKernel reported an error */
};

/* A (batch, seq, head, dim) view: element pointer + element strides; dim stride is 1. */
/* Launch flags (usp_fwd_args.flags / usp_bwd_args.flags).
 * USP_LAUNCH_INTERLEAVE: other kernels -- RCCL's send/recv and all-to-all kernels on another stream -- must
 * be able to start WHILE this launch runs.  By default the flash kernels are persistent: one workgroup per
 * CU for the whole launch, each holding the CU's entire register file, so nothing else can be scheduled
 * until the launch ends (fastest when the GPU does nothing else: +4 % forward).  With this flag one
 * workgroup per work item is launched instead; CUs free up every few microseconds and a collective queued
 * on another stream gets its workgroups resident at once.  Use it whenever a transfer is meant to overlap
 * the kernel (ring steps, pipelined Ulysses exchange). */
#define USP_LAUNCH_INTERLEAVE 1
/* USP_ATTN_WINDOW (ABI v5): the window_left / window_right fields are valid (without the bit they are ignored, so a
 * zero-initialised struct means "no window", not "window (0, 0)"). */
#define USP_ATTN_WINDOW 2
/* Kernel-family selectors (ABI v6; usp_flash_fwd / usp_flash_bwd).  The library holds two families of flash kernels: the
 * one-wave-per-SIMD family (a wave owns 64 rows / keys and its SIMD's whole register file: usp_flash_fwd64.hip,
 * usp_flash_bwd64.hip, usp_flash_bwd_dq64.hip) and the two-waves-per-SIMD family (32 rows per wave, 8 or 4 waves:
 * usp_flash_fwd.hip, usp_flash_bwd.hip), and picks per launch.  With one of these bits the caller picks -- per CALL, not
 * per process -- which is what lets a parity test pin the kernel it means to test, and a bench time both families on
 * the same box:
 *   USP_FORCE_ROW64   every flash kernel of the call must come from the 64-row family; a call that family does not
 *                     serve (head dim != 128, packed batch, window) returns USP_EUNSUPPORTED and launches nothing
 *                     (unforced, the library picks the 64-row forward K split only for long cuts);
 *   USP_FORCE_WAVE32  every flash kernel of the call comes from the 32-rows-per-wave family.
 * Both bits at once: USP_EINVAL.  usp_last_launch_kinds() reports what a call actually launched.
 * The library reads no environment variable: a call's behaviour comes from its argument block alone.
 * Layouts the 64-row family serves (beyond the alignment every call needs): its LDS-DMA pieces XOR a swizzle into a per-lane
 * byte offset whose row part must be a multiple of 256 bytes, and address 64 rows by 32-bit offsets, so
 *   forward            k.stride_s % 128 == 0 (elements);  k.stride_s, v.stride_s < 2^24   (v.stride_s % 128 is NOT needed:
 *                      the V pieces' offsets are sums -- tests/test_gpu_layouts.py::test_row64_stride_conditions_forward);
 *   backward, dQ       k.stride_s % 128 == 0 and v.stride_s % 128 == 0;  both < 2^24;
 *   backward, dK/dV    q.stride_s % 128 == 0 and dout.stride_s % 128 == 0;  both < 2^24   (either 16-bit type, any softmax_scale: K
 *                      is never multiplied by the scale in the 16-bit type -- tests/test_gpu_range.py::test_fp16_edge).
 * Any other layout: USP_EUNSUPPORTED with USP_FORCE_ROW64 (nothing is launched or written), the other family's kernel for
 * that launch without it.  The 32-rows-per-wave family takes every aligned layout, with one bound: its dK/dV kernel
 * addresses the rows of a head by a 32-bit byte offset, so Sq * q.stride_s * 2 and Sq * dout.stride_s * 2 must stay below
 * 2^31 (USP_EUNSUPPORTED at or above it, when the 64-row dK/dV kernel does not take the launch).
 * Pinned by tests/test_gpu_layouts.py (test_row64_stride_conditions_*, test_wave8_dkdv_32bit_offset_bound). */
#define USP_FORCE_ROW64 4
#define USP_FORCE_WAVE32 8
/* usp_flash_bwd only (ABI v6): issue only one of the backward's two launches -- the dK/dV launch (+ its head / cut reduce)
 * or the dQ launch (+ its cut reduce).  The two are independent given (lse, delta); a caller may order them around its
 * transfers (dK/dV travel the ring, dQ stays), and a bench can time each kernel alone with stream events.  The skipped
 * launch's outputs are not touched.  Both bits at once: USP_EINVAL. */
#define USP_BWD_SKIP_DQ 16
#define USP_BWD_SKIP_DKDV 32
/* USP_ATTN_SOFTCAP: tanh logit soft-capping as flash-attn defines it (`softcap`, passed through by the reference's block
 * calls, e.g. yunchang/ring/zigzag_ring_flash_attn.py:29-43): the `softcap` field is valid and every score S (softmax_scale
 * already applied) is replaced by cap * tanh(S / cap) before the causal / window / ragged mask.  Without the bit the field
 * is ignored (a binding built before it never sets the bit, so the library never reads past that binding's struct).
 * With the bit, a softcap that is not a finite number > 0 is USP_EINVAL; with USP_FORCE_ROW64 it is USP_EUNSUPPORTED (the
 * 64-row family declines it; unforced, such calls run on the two-waves-per-SIMD kernels).  usp_attn_features() tells a
 * binding whether the library it loaded serves the bit. */
#define USP_ATTN_SOFTCAP 64
/* USP_ATTN_SHIFT: the `mask_shift` field is valid and the diagonal of the mask moves by it: (Sk - Sq) is replaced by
 * (Sk - Sq + mask_shift) in the causal bound and in both window bounds, so query row i sees key j iff
 *     i + (Sk - Sq + mask_shift) - window_left <= j <= i + (Sk - Sq + mask_shift) + window_right      (causal: window_right = 0)
 * -- the mask of ONE block of a sequence that is split over a ring (the reference has no such argument: it hands the same
 * `window_size` to every block, yunchang/ring/ring_flash_attn.py:36-48, which is a different function).  Any value with
 * |mask_shift| < 2^30 is served (USP_EINVAL beyond): rows, or a whole launch, that see no key give out = 0, lse = -inf and
 * zero gradients, as an empty row does without the bit.  A shift with neither `causal` nor a window bounds nothing and is
 * ignored by the mask; with ALiBi (usp_flash_fwd_alibi / usp_flash_bwd_alibi) it still moves the bias, whose distances are
 * measured from the same diagonal.  Dense launches only: a packed batch with the bit is USP_EUNSUPPORTED.  The 64-row family serves a shifted launch
 * exactly where it serves the same launch unshifted (no left window bound).
 * Served range: window_left and window_right may be ANY int32 (INT32_MAX as "unbounded" included), with or without a shift;
 * the bounds are formed in 64 bits (csrc/usp_mask_decode.h).  A bound that cuts no (row, key) pair of the launch at this
 * (Sq, Sk, mask_shift) is dropped -- the launch is then served as the same launch without that bound, by every family that
 * serves that one, a left bound that cuts nothing included -- and a bound that cuts every pair gives the empty result above.
 * The kernels' own index arithmetic needs Sq + Sk < 2^29.  Without the bit the field is ignored; a binding
 * built before it never sets the bit, and the field lies in what was padding (behind softmax_scale), so such a binding's struct
 * has the same size and offsets and is never read past; usp_attn_features() reports the bit. */
#define USP_ATTN_SHIFT 128
/* USP_ATTN_ALIBI: a FEATURE bit, reported by usp_attn_features() and not read from args->flags: the library exports
 * usp_flash_fwd_alibi / usp_flash_bwd_alibi (below), which take flash-attn's `alibi_slopes` beside the unchanged argument
 * blocks (ABI still v7: no struct, field or version changed). */
#define USP_ATTN_ALIBI 256
/* USP_ATTN_DROPOUT: a FEATURE bit like USP_ATTN_ALIBI: the library exports usp_flash_fwd_dropout / usp_flash_bwd_dropout (below),
 * which take flash-attn's `dropout_p` and a seed beside the unchanged argument blocks (ABI still v7). */
#define USP_ATTN_DROPOUT 512
/* USP_ATTN_SINK: a FEATURE bit like USP_ATTN_ALIBI: the library exports usp_flash_fwd_sink / usp_sink_bwd (below), which take a
 * learned per-head sink logit beside the unchanged argument blocks (ABI still v7). */
#define USP_ATTN_SINK 1024
/* USP_ATTN_DOC: a FEATURE bit like USP_ATTN_ALIBI: the library exports usp_flash_fwd_doc / usp_flash_bwd_doc (below), which take a
 * per-row left key bound (the document mask of packed pre-training sequences) beside the unchanged argument blocks (ABI still v7). */
#define USP_ATTN_DOC 2048
/* USP_ATTN_SPAN: a FEATURE bit like USP_ATTN_DOC: the library exports usp_flash_fwd_span / usp_flash_bwd_span (below), which take a
 * per-row right key bound beside the document's left one (bidirectional spans: prefix-LM blocks, packed bidirectional documents)
 * beside the unchanged argument blocks (ABI still v7). */
#define USP_ATTN_SPAN 4096
/* USP_ATTN_BLOCK_MASK: a FEATURE bit like USP_ATTN_DOC: the library exports usp_block_list_bytes / usp_flash_fwd_bsp /
 * usp_flash_bwd_bsp (below), which take a 128 x 128 block mask beside the unchanged argument blocks. */
#define USP_ATTN_BLOCK_MASK 8192
/* USP_ATTN_MAX_LOGIT: a FEATURE bit like USP_ATTN_SINK: the library exports usp_flash_fwd_maxlogit / usp_row_max_reduce (below),
 * which return the largest visible pre-softmax logit of every row / head beside the unchanged argument blocks (ABI still v7). */
#define USP_ATTN_MAX_LOGIT 16384
/* USP_ATTN_BLOCK_SELECT: a FEATURE bit like USP_ATTN_BLOCK_MASK: the library exports usp_block_means / usp_block_select (below),
 * which produce a 128 x 128 block mask on the device -- top-k of mean-pooled blocks -- for usp_flash_fwd_bsp / usp_flash_bwd_bsp
 * (ABI still v7). */
#define USP_ATTN_BLOCK_SELECT 32768
/* USP_ATTN_BLOCK_SELECT_TOP_P: a FEATURE bit like USP_ATTN_BLOCK_SELECT: the library exports usp_block_select_top_p (below), which
 * selects the block mask by cumulative softmax mass of the pooled scores in place of a fixed count (ABI still v7). */
#define USP_ATTN_BLOCK_SELECT_TOP_P 65536
/* USP_ATTN_BLOCK_MASS: a FEATURE bit like USP_ATTN_BLOCK_SELECT: the library exports usp_block_attn_mass (below), which returns the
 * block-pooled attention map of a call -- the share of the softmax mass every 128 x 128 block holds (ABI still v7; the value is
 * no flag of an argument block, where it means USP_DKDV_KEYS128). */
#define USP_ATTN_BLOCK_MASS 131072
/* Item width of the 64-row family's dK/dV launch (usp_flash_bwd only; selectors like USP_FORCE_*, per call).  That launch
 * exists in two forms, both noted as USP_KIND_DKDV_ROW64:
 *   USP_DKDV_KEYS128  flash_bwd_dkdv64_kernel: a work item owns 128 keys, two waves share a 64-key slice (S, P, dV | dP, dS, dK);
 *   USP_DKDV_KEYS256  flash_bwd_dkdv64u_kernel: a work item owns 256 keys, each wave does all four products for its 64 keys --
 *                     Q / dO are streamed half as often and P never crosses LDS; a short causal range pays more masked
 *                     tiles per item and has half the items.  At equal dkdv_heads, dK / dV are bit-identical between the two for
 *                     uncut launches and for cut launches without a causal bound; a cut causal launch cuts the second 128
 *                     keys of a 256-key block at other query tiles than the 128-key item that owns them, so their fp32
 *                     partial sums group differently there (tests/test_gpu_dkdv256.py).
 * With neither bit the library picks per launch (csrc/usp_flash_bwd.hip: dkdv_keys_of); dkdv_heads = 0 and the workspace size
 * follow the width, so ask usp_flash_bwd_workspace_bytes with the same flags.  With a bit, a call whose dK/dV launch the
 * 64-row family does not serve (head dim != 128, packed batch, window, softcap, one of the extra entry points' features, a layout
 * above) returns USP_EUNSUPPORTED and launches nothing; a call that skips the dK/dV launch ignores the bits.  Both bits at once,
 * or one of them with USP_FORCE_WAVE32: USP_EINVAL.  USP_KIND_DKDV_KEYS256 in usp_last_launch_kinds() says which form ran. */
#define USP_DKDV_KEYS256 65536
#define USP_DKDV_KEYS128 131072

typedef struct usp_tensor {
  void* ptr;
  int64_t stride_b, stride_s, stride_h;
} usp_tensor;

/* ----------------------------------------------------------------------------------------------
 * Blockwise flash-attention forward, with the ring LSE-merge fused into the epilogue.
 *
 * Replaces the `fwd-only` callable: pytorch_attn_forward(op_type="efficient")
 * (yunchang/kernels/attention.py:44-136, aten op at :76-86) / flash_attn_forward (:165-202), as
 * called by the ring schedules (yunchang/ring/zigzag_ring_flash_attn.py:29-43,
 * yunchang/ring/ring_flash_attn.py:36-48), AND the update_out_and_lse that follows each call
 * (yunchang/ring/utils.py:10-51; slice form used at zigzag_ring_flash_attn.py:61-67).
 *
 * Computes, for q (B,Sq,Hq,D), k/v (B,Sk,Hkv,D) [GQA: q head i uses kv head i / (Hq/Hkv)]:
 *     S = q k^T * softmax_scale ; causal: key j visible to query i iff j <= i + (Sk - Sq)
 *     USP_ATTN_SOFTCAP: S <- softcap * tanh(S / softcap)          (before the mask)
 *     blk_lse = logsumexp_j S ;  blk_out = softmax(S) v          (fp32 accumulate)
 * then, per query row i of this call:
 *     merge_in != 0 : (o, lse) = merge((acc[i], lse[i]), (blk_out, blk_lse))   [utils.py:25-26]
 *     merge_in == 0 : (o, lse) = (blk_out, blk_lse)
 *     lse[i] <- lse                                   (fp32, natural log; -inf for an empty row)
 *     i in [final_begin, final_end) : out[i] <- o rounded to `dtype`   (needs out.ptr != NULL)
 *     otherwise                      : acc[i] <- o  (fp32)             (needs acc.ptr != NULL)
 * `lse` is (B,Hq,Sq) with seq stride 1.  A single non-ring call uses merge_in=0,
 * final_begin=0, final_end=Sq, acc.ptr=NULL.
 *
 * Packed variable-length batches (replaces _flash_attn_varlen_forward as called at
 * yunchang/ring/zigzag_ring_flash_attn_varlen.py:88-112 and ring_flash_attn_varlen.py:56-71, the
 * k[half_index0] / q[half_index1] gathers at zigzag_ring_flash_attn_varlen.py:127-140, and the LSE
 * (un)flatten of yunchang/ring/utils.py:96-117): seq_q / seq_k point to B (first_row, rows) int32
 * pairs in DEVICE memory.  q/out/acc are (T,Hq,D) and k/v (T',Hkv,D) row-major token tensors
 * (stride_b ignored); sequence b attends rows [first, first+rows) of each side, causal alignment per
 * sequence; lse is (Hq,T): lse[h*lse_stride_h + row].  Sq / Sk are the MAXIMUM rows over the batch
 * (they size the launch).  Sequences with 0 query rows are skipped; a sequence with 0 key rows gives
 * blk_out = 0, blk_lse = -inf.  A (first,rows) pair may address any sub-range of the token tensors,
 * e.g. the front or back half of every sequence -- no gather copies are needed.  In this mode
 * final_begin / final_end count HALF sequences (0, 1 or 2): rows [final_begin*rows/2,
 * final_end*rows/2) of every sequence are final (2 = to the end).
 * `sched` (packed mode only, optional): 16 int32 of device memory, ZEROED ONCE by the caller.  With it
 * the workgroups pull work items from a dynamic queue (heaviest first, empty items of short sequences
 * skipped), which is what balances batches of unequal sequences; without it they walk static lists,
 * which is only balanced when all sequences are equally long.  The kernels leave the block zeroed;
 * launches that may run concurrently (different streams) must not share one block.
 * -------------------------------------------------------------------------------------------- */
typedef struct usp_fwd_args {
  int32_t dtype;                 /* USP_BF16 | USP_FP16: element type of q,k,v,out */
  int32_t B, Sq, Sk, Hq, Hkv, D;
  int32_t causal;                /* 0 | 1 (bottom-right aligned) */
  float softmax_scale;           /* > 0 */
  int32_t mask_shift;            /* read only with USP_ATTN_SHIFT in `flags`: added to (Sk - Sq) in every mask bound (see the
                                    flag).  It occupies the four bytes that used to be padding in front of the 8-byte aligned
                                    `q`: every other offset and sizeof are those of ABI v7's first release */
  usp_tensor q, k, v;            /* inputs */
  usp_tensor out;                /* 16-bit output rows (final rows only); ptr may be NULL */
  usp_tensor acc;                /* fp32 running output; ptr may be NULL */
  float* lse;                    /* fp32 running / final logsumexp */
  int64_t lse_stride_b, lse_stride_h;
  int32_t merge_in;              /* 0 | 1 */
  int32_t final_begin, final_end;/* row range of this call whose result is final */
  const int32_t* seq_q;          /* packed variable-length batch (both NULL = dense), see below */
  const int32_t* seq_k;
  int32_t* sched;                /* packed mode, optional: 64-byte device control block, see below */
  int32_t flags;                 /* USP_LAUNCH_* bits */
  int32_t k_splits;              /* dense mode, optional: cut every query tile's keys into this many work items
                                    (2..8; 0 or 1 = off); needs `workspace`, see usp_flash_fwd_workspace_bytes() */
  void* workspace;               /* device scratch of usp_flash_fwd_workspace_bytes(args, k_splits) bytes, 16-byte
                                    aligned; NULL = no split */
  int32_t window_left, window_right; /* read only with USP_ATTN_WINDOW in `flags` (ABI v5): sliding-window (local)
                                    attention as flash-attn defines it (kernels/attention.py:165-202 passes
                                    `window_size` through): query row i sees key j iff
                                    i + (Sk - Sq) - window_left <= j <= i + (Sk - Sq) + window_right; a negative value =
                                    unbounded on that side; `causal` caps window_right at 0 */
  float softcap;                 /* read only with USP_ATTN_SOFTCAP in `flags`: finite, > 0 (see the flag) */
} usp_fwd_args;

int usp_flash_fwd(const usp_fwd_args* args, void* stream);

/* K split (dense launches): a launch with few (batch, head, 256-row tile) work items cannot fill 256 CUs, and a causal
 * one lasts as long as its heaviest item (measured on MI355X, B1 S16384 D128 causal: 2 heads 548 TFLOP/s, 4 heads 891,
 * 8 heads 1133; the same 2 / 4 heads cut in two along K: 833-857 / 1093 -- profiles/r02_kbench_split.log).  With
 * k_splits = n and a workspace every item becomes n items over equal runs of the K tiles it sees; each writes a
 * normalised fp32 partial + LSE to the workspace and a second, HBM-bound launch on the same stream combines them [and
 * the running result when merge_in] into exactly the outputs described above (results equal up to fp32 summation
 * order).  Returns the bytes needed: n * (B*Sq*Hq*D + B*Hq*Sq) * 4; 0 for n <= 1 or a packed batch. */
int64_t usp_flash_fwd_workspace_bytes(const usp_fwd_args* args, int32_t k_splits);

/* ----------------------------------------------------------------------------------------------
 * Blockwise flash-attention backward.
 *
 * Replaces the `bwd-only` callable flash_attn_backward (yunchang/kernels/attention.py:205-250;
 * the TORCH_* variant pytorch_attn_backward :138-159 raises), as called at
 * zigzag_ring_flash_attn.py:115-137 / ring_flash_attn.py:102-122, AND the fp32 accumulation the
 * ring schedule performs on its results (zigzag_ring_flash_attn.py:147-170).
 *
 * Inputs: dout,q (B,Sq,Hq,D); k,v (B,Sk,Hkv,D); lse (B,Hq,Sq) = the GLOBAL logsumexp of the rows
 * (not this block's); delta (B,Hq,Sq) = rowsum(dout * out_global) from usp_bwd_delta().
 *     P = exp(S - lse) ; dV = P^T dO ; dP = dO V^T ; dS = P * (dP - delta) * scale
 *     dQ = dS K ; dK = dS^T Q                  (GQA: dK,dV summed over the Hq/Hkv query heads)
 * USP_ATTN_SOFTCAP: with t = tanh(S / softcap), S = q k^T * softmax_scale:
 *     P = exp(softcap * t - lse) ; dS = P * (dP - delta) * (1 - t^2) * scale   (the rest as above)
 * Outputs are fp32 (B,S,H,D) tensors: dq (+)= dQ, dk (+)= dK, dv (+)= dV, where "+=" is used when
 * the matching accum_* flag is non-zero and "=" otherwise.  Deterministic (no atomics).
 * `workspace` (optional) enables the GQA head split described at usp_flash_bwd_workspace_bytes().
 *
 * Packed variable-length batches (replaces _flash_attn_varlen_backward as called at
 * yunchang/ring/zigzag_ring_flash_attn_varlen.py:208-231 / ring_flash_attn_varlen.py:125-147, the
 * half-index gathers / scatters around it (:246-264) and get_half_lse (:45-58)): seq_q / seq_k as in
 * usp_fwd_args -- B (first_row, rows) pairs in device memory; dout/q/dq/dq16 are (T,Hq,D) token
 * tensors addressed through seq_q, k/v/dk/dv/dk16/dv16 (T',Hkv,D) through seq_k, lse/delta are
 * (Hq,T); Sq / Sk are the maximum rows over the batch.  Gradient rows outside every sequence's
 * range are not touched; sequences with 0 rows on either side are skipped entirely.
 * -------------------------------------------------------------------------------------------- */
typedef struct usp_bwd_args {
  int32_t dtype;
  int32_t B, Sq, Sk, Hq, Hkv, D;
  int32_t causal;
  float softmax_scale;
  int32_t mask_shift;            /* as in usp_fwd_args, in the same former padding; read only with USP_ATTN_SHIFT in `flags` */
  usp_tensor dout, q, k, v;      /* 16-bit inputs */
  const float* lse;              /* (B,Hq,Sq), seq stride 1 */
  const float* delta;            /* (B,Hq,Sq), seq stride 1 */
  int64_t lse_stride_b, lse_stride_h;
  int64_t delta_stride_b, delta_stride_h;
  usp_tensor dq, dk, dv;         /* fp32 outputs / accumulators */
  int32_t accum_dq, accum_dk, accum_dv;
  usp_tensor dq16, dk16, dv16;   /* optional 16-bit FINAL outputs (ptr may be NULL): when set, the
                                    result ((accum ? X : 0) + block) is rounded to `dtype` and stored
                                    there instead of being written back to the fp32 tensor X */
  void* workspace;               /* optional scratch (device, 16-byte aligned), see below; may be NULL */
  int64_t workspace_bytes;
  const int32_t* seq_q;          /* packed variable-length batch (both NULL = dense), see below */
  const int32_t* seq_k;
  int64_t total_k;               /* packed mode: rows of the k/v/dk/dv token tensors (sizes the workspace) */
  int32_t* sched;                /* packed mode, optional: 64-byte device control block (as usp_fwd_args) */
  int32_t flags;                 /* USP_LAUNCH_* / USP_ATTN_* bits */
  int32_t dq_splits;             /* dense mode, optional (ABI v5): cut every (head, 256-row query block) item of the dQ
                                    launch into this many items along the keys it sees (2..8; 0 / 1 = off) */
  int32_t dkdv_splits;           /* ... and every (query head, 128-key block) item of the dK/dV launch along the query
                                    rows that see it.  Both need `workspace`, see usp_flash_bwd_workspace_bytes() */
  int32_t window_left, window_right; /* as usp_fwd_args; read only with USP_ATTN_WINDOW in `flags` */
  int32_t dkdv_heads;            /* GQA, dense or packed (ABI v7): query heads of a KV group that ONE dK/dV work item streams
                                    into its accumulators -- a divisor of Hq/Hkv (else USP_EINVAL).  Hq/Hkv = the whole group
                                    inside the workgroup (no per-head partials, no reduce launch); 1 = one item per query
                                    head; 0 = the library decides (see usp_flash_bwd_workspace_bytes()) */
  float softcap;                 /* as usp_fwd_args; read only with USP_ATTN_SOFTCAP in `flags` */
} usp_bwd_args;

int usp_flash_bwd(const usp_bwd_args* args, void* stream);

/* ----------------------------------------------------------------------------------------------
 * ALiBi: usp_flash_fwd / usp_flash_bwd with flash-attn's `alibi_slopes` (forwarded by the reference to every block call,
 * yunchang/kernels/attention.py:165-250).  For query head h of batch b with slope m = alibi_slopes[b * alibi_stride_b + h]
 * (DEVICE fp32, h < Hq; alibi_stride_b = 0: one (Hq,) vector for the whole batch):
 *     S[i, j] = softmax_scale * q_i . k_j  -  m * | i + (Sk - Sq + shift) - j |       shift = mask_shift with USP_ATTN_SHIFT, else 0
 * and the causal / window / ragged mask is applied after.  At shift = 0 this is flash-attn's definition; with the shift of a ring
 * block the distances are those of GLOBAL positions (the reference hands the same slopes to every block and so measures them
 * inside each block: a different function).  `lse` is the true logsumexp of these biased scores (flash-attn's causal shortcut
 * adds m * j instead, which moves its LSE per row; the ring merges by LSE, so that is not copied).  Backward: P = exp(S - lse);
 * dS, dQ, dK, dV as without the bias, which is additive and has no gradient path to q, k or v.  The slopes get no gradient.
 * alibi_slopes == NULL is exactly usp_flash_fwd / usp_flash_bwd: the same kernels, bit-identical results.  Everything else is as
 * the argument block says (k_splits, dq_splits, dkdv_splits, dkdv_heads and the workspace functions, merge_in and the final
 * rows, USP_LAUNCH_INTERLEAVE, USP_ATTN_WINDOW, USP_ATTN_SHIFT, USP_BWD_SKIP_*).  With non-NULL slopes:
 *   - a negative alibi_stride_b is USP_EINVAL;
 *   - USP_ATTN_SOFTCAP, a packed batch (seq_q / seq_k) and USP_FORCE_ROW64 are USP_EUNSUPPORTED, nothing launched or written;
 *   - every head dim runs on the two-waves-per-SIMD family (ALiBi instantiations of its kernels; unforced D = 128 included, as
 *     for softcap); usp_last_launch_kinds() reports the wave8 / wave4 / split-merge / reduce bits that were launched.
 * -------------------------------------------------------------------------------------------- */
int usp_flash_fwd_alibi(const usp_fwd_args* args, const float* alibi_slopes, int64_t alibi_stride_b, void* stream);
int usp_flash_bwd_alibi(const usp_bwd_args* args, const float* alibi_slopes, int64_t alibi_stride_b, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Dropout: usp_flash_fwd / usp_flash_bwd with flash-attn's `dropout_p` (forwarded by the reference to every block call; its ring
 * backward passes rng_state=None, yunchang/ring/ring_flash_attn.py:112-119, and so differentiates another mask than its forward
 * applied).  Here the mask is a PURE FUNCTION OF GLOBAL POSITIONS (csrc/usp_dropout_rng.h), so forward and backward, any kernel,
 * any tiling and any block of a ring regenerate the same one.  For drop probability p, 64-bit seed and the global position
 * (row0, key0, head0) of the launch's row 0, key 0 and QUERY head 0:
 *     t    = min(256, max(1, lrintf((1 - p) * 256)))          keep threshold; the realised keep probability is t / 256
 *     i    = row0 + local query row    j = key0 + local key    h = head0 + local QUERY head    b = batch index   (all uint32)
 *     w[4] = Philox4x32-10(counter = (i >> 2, j >> 2, h, b), key = (seed & 0xffffffff, seed >> 32))
 *     keep(i, j) = ((w[i & 3] >> (8 * (j & 3))) & 0xff) < t
 * (standard Philox constants: multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments 0x9E3779B9 / 0xBB67AE85, 10 rounds; one call
 * gives the 16 keep bytes of a 4-row x 4-key patch: word = row, byte = key).  With P the softmax probabilities of the masked
 * scores (causal / window / shift exactly as without dropout):
 *     lse_i = logsumexp_j S_ij                              -- unchanged by dropout
 *     out_i = (256/t) * sum_j keep_ij P_ij v_j
 *     delta_i = rowsum(dout_i * out_i)                       -- usp_bwd_delta, unchanged, on the dropped `out`
 *     dV_j  = (256/t) * sum_i keep_ij P_ij dO_i
 *     dS_ij = P_ij * ((256/t) * keep_ij * (dO_i . v_j) - delta_i) * scale ;   dQ = dS K ;   dK = dS^T Q     (GQA sums as ever)
 * The rescale is by the REALISED rate 256/t, not 1/(1-p).  `lse` is that of the un-dropped scores and `out` is linear in the
 * kept terms, so the ring's LSE merge and the K-split merge are unchanged.  The mask is this library's own: it is not
 * flash-attn's, which is tied to that kernel's tile layout.
 *   - p_drop == 0, or a p_drop whose threshold is 256, is exactly usp_flash_fwd / usp_flash_bwd: the same kernels, bit-identical
 *     results, the offsets ignored;
 *   - a p_drop that is NaN, negative or >= 1, or a negative row0 / key0 / head0, is USP_EINVAL;
 *   - row0 % 4 != 0, key0 % 4 != 0, row0 + Sq or key0 + Sk >= 2^31, USP_ATTN_SOFTCAP, a packed batch (seq_q / seq_k) and
 *     USP_FORCE_ROW64 are USP_EUNSUPPORTED, nothing launched or written;
 *   - every head dim runs on the two-waves-per-SIMD family (dropout instantiations of its kernels, as for softcap and ALiBi);
 *     usp_last_launch_kinds() reports the wave8 / wave4 / split-merge / reduce bits that were launched.
 * Everything else is as the argument block says (k_splits, dq_splits, dkdv_splits, dkdv_heads and the workspace functions,
 * merge_in and the final rows, USP_LAUNCH_INTERLEAVE, USP_ATTN_WINDOW, USP_ATTN_SHIFT, USP_BWD_SKIP_*, GQA).  Dropout together with
 * ALiBi has no entry point.  The seed is a launch argument: a captured graph replays the mask it was captured with.
 * -------------------------------------------------------------------------------------------- */
int usp_flash_fwd_dropout(const usp_fwd_args* args, float p_drop, uint64_t seed, int32_t row0, int32_t key0, int32_t head0,
                          void* stream);
int usp_flash_bwd_dropout(const usp_bwd_args* args, float p_drop, uint64_t seed, int32_t row0, int32_t key0, int32_t head0,
                          void* stream);

/* ----------------------------------------------------------------------------------------------
 * Attention sinks: usp_flash_fwd with a learned per-head sink logit (GPT-OSS `sinks`, flash-attn 3's `s_aux` / learnable sink;
 * "off-by-one softmax" at 0).  sinks[h] (DEVICE fp32, h < Hq) joins the softmax denominator of every row of query head h and
 * carries no value.  It is in SCORE units: compared with softmax_scale * q.k after the mask, NOT multiplied by softmax_scale.
 * With S_ij the visible scores of row i (causal / window / shift exactly as without sinks) and s = sinks[h]:
 *     lse_i   = log( exp(s) + sum_j exp(S_ij) )              ( = s for a row that sees no key; never -inf )
 *     P_ij    = exp(S_ij - lse_i)                            ( rows sum to 1 - p_sink,i ,  p_sink,i = exp(s - lse_i) )
 *     out_i   = sum_j P_ij v_j                               ( 0 for a row that sees no key )
 *     delta_i = rowsum(dout_i * out_i)                       -- usp_bwd_delta, unchanged
 *     dS_ij   = P_ij * (dP_ij - delta_i) * scale ;  dQ, dK, dV as ever
 *     ds_h    = - sum_{b,i} exp(s_h - lse_{b,h,i}) * delta_{b,h,i}                                         -- usp_sink_bwd
 * The returned `lse` INCLUDES the sink (flash-attn's convention for s_aux): it is what a ring merges by and all the backward
 * needs.  There is no usp_flash_bwd_sink: usp_flash_bwd, handed this lse, IS the backward for dQ, dK and dV (its kernels only
 * ever need P = exp(S - lse)), and usp_sink_bwd gives the sink's own gradient from the same (lse, delta).
 * The sink is position-free and must be counted ONCE per row: it belongs to the launch that opens the rows' running state
 * (merge_in == 0).  Later merge_in launches over further keys, and the K-split merge, then work unchanged on an lse that
 * already holds it.  In the kernels it is the epilogue's merge with the constant block (o = 0, lse = s): no extra pass.
 *   - sinks == NULL is exactly usp_flash_fwd: the same kernels, bit-identical results;
 *   - with sinks, merge_in != 0 is USP_EINVAL;
 *   - with sinks, USP_ATTN_SOFTCAP, a packed batch (seq_q / seq_k) and USP_FORCE_ROW64 are USP_EUNSUPPORTED, nothing launched
 *     or written (these checks follow the argument checks every call gets, as for ALiBi and dropout);
 *   - every head dim runs on the two-waves-per-SIMD family (flash_fwd_sink_kernel: the plain family's tile loops, pipelined
 *     interior tiles included, with the sink in the epilogue; unforced D = 128 included); usp_last_launch_kinds() reports the
 *     wave8 / wave4 / split-merge bits that were launched.
 * Everything else is as the argument block says (k_splits and the workspace -- partial 0 carries the sink --, final_begin /
 * final_end with acc, USP_LAUNCH_INTERLEAVE, USP_ATTN_WINDOW, USP_ATTN_SHIFT, GQA, any aligned layout).  Sinks together with
 * ALiBi or dropout have no entry point.
 *
 * usp_sink_bwd: dsinks[h] (+)= - sum_{b < B, i < S} exp(sinks[h] - lse[b,h,i]) * delta[b,h,i]  for h < H, "+=" with accum != 0.
 * lse / delta are (B,H,S) fp32 with seq stride 1 and the given batch / head strides; sinks and dsinks are (H,) fp32.  A term
 * whose lse is -inf counts as 0.  fp32, deterministic (one workgroup per head, a fixed summation order, no atomics).  Null
 * pointers and non-positive sizes are USP_EINVAL.
 * A sink is a parameter REPLICATED over a sequence-parallel group: each rank calls this on its own rows (ring) or heads
 * (Ulysses) and so holds its SHARE of the gradient; the sum over the group is the gradient, as for any replicated parameter.
 * Nothing in this library reduces it across ranks.
 * -------------------------------------------------------------------------------------------- */
int usp_flash_fwd_sink(const usp_fwd_args* args, const float* sinks, void* stream);
int usp_sink_bwd(int32_t B, int32_t S, int32_t H, const float* sinks, const float* lse, int64_t lse_stride_b,
                 int64_t lse_stride_h, const float* delta, int64_t delta_stride_b, int64_t delta_stride_h, float* dsinks,
                 int32_t accum, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Max logits: usp_flash_fwd that also returns, per query row, the largest pre-softmax logit the row sees (QK-clip / MuonClip
 * need the per-head maximum at every step; TransformerEngine's `return_max_logit`).  With S_ij = softmax_scale * q_i . k_j:
 *     row_max[b, h, i] = max over the keys j row i SEES of S_ij          ( -inf for a row that sees no key )
 * in SCORE units, the unit `sinks` uses.  The mask is the call's own (causal, ragged Sk, USP_ATTN_WINDOW, USP_ATTN_SHIFT): a
 * hidden key never counts.  `row_max` is DEVICE fp32, element (b, h, i) at b * stride_b + h * stride_h + i (seq stride 1, like
 * lse); rows i < Sq are written, with ordinary stores, nothing else.  out, acc and lse are bit for bit those of usp_flash_fwd on
 * the two-waves-per-SIMD kernels.  The value is the TRUE maximum, not the online softmax's reference (which the pipelined loop
 * raises lazily): every score is one fp32 MFMA chain over D, so the result does not depend on the tiling, and
 *     |row_max - exact| <= 2 * softmax_scale * D * 2^-24 * sum_d |q_d k_d| + 2^-23 |exact|.
 * The maximum is row-local and position-free and travels with lse: the launch that opens the rows' running state
 * (merge_in == 0) writes it, a merge_in launch over further keys takes the maximum with the value already there.
 *   - row_max == NULL is exactly usp_flash_fwd: the same kernels, bit-identical results, whatever the strides;
 *   - a negative stride (or a row_max off a 4-byte boundary) is USP_EINVAL;
 *   - USP_ATTN_SOFTCAP, a packed batch (seq_q / seq_k) and USP_FORCE_ROW64 are USP_EUNSUPPORTED, nothing launched or written
 *     (these checks follow the argument checks every call gets, as for the sinks);
 *   - k_splits is IGNORED, as under the document mask: the launch is served uncut, never refused;
 *   - every head dim runs on the two-waves-per-SIMD family (flash_fwd_maxl_kernel: the plain family's tile loops, pipelined
 *     interior tiles included, at one v_max per tile; unforced D = 128 included); usp_last_launch_kinds() reports wave8 / wave4.
 * Everything else is as the argument block says (final_begin / final_end with acc, USP_LAUNCH_INTERLEAVE, GQA, any aligned
 * layout).  The backward is untouched.  Max logits together with ALiBi, dropout, sinks, documents, spans or a block mask have no
 * entry point.
 *
 * usp_row_max_reduce: out[h] = max_{b < B, i < S} row_max[b,h,i] for h < H; with accum != 0 the maximum with out[h] as well.
 * row_max is (B,H,S) fp32 with seq stride 1 and the given batch / head strides; out is (H,) fp32.  Exact and deterministic (one
 * workgroup per head, no atomics).  Null pointers, non-positive sizes and negative strides are USP_EINVAL.
 * Over a sequence-parallel group each rank holds its SHARE -- the maximum over its own rows (ring) or heads (Ulysses); the MAX
 * over the group is the value.  Nothing in this library reduces it across ranks.
 * -------------------------------------------------------------------------------------------- */
int usp_flash_fwd_maxlogit(const usp_fwd_args* args, float* row_max, int64_t row_max_stride_b, int64_t row_max_stride_h,
                           void* stream);
int usp_row_max_reduce(int32_t B, int32_t S, int32_t H, const float* row_max, int64_t row_max_stride_b,
                       int64_t row_max_stride_h, float* out, int32_t accum, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Document mask: usp_flash_fwd / usp_flash_bwd with a left key bound read per row.  A sequence that packs several documents must
 * keep every row from attending across a document boundary; for one launch (a whole sequence, or one block of a ring) that is
 *     row i sees key j   iff   j >= row_lo[i]   and   the mask of the argument block (causal, ragged Sk) lets it,
 * with row_lo (HOST-computed, DEVICE int32, (Sq,) per batch entry: row i of batch b at row_lo[b * row_lo_stride_b + i]; stride 0:
 * one array for the whole batch; the arrays are shared by all heads) in the LAUNCH'S OWN key numbering: row_lo[i] in [0, Sk] is
 * the first key row i sees, Sk = it sees none.  The backward's dK/dV launch owns keys and takes the transpose,
 *     key_hi[j] in [0, Sq] = one past the last row that sees key j under this bound  ( = #{ i : row_lo[i] <= j } ),
 * (Sk,) per batch entry with key_hi_stride_b.  BOTH ARRAYS MUST BE NON-DECREASING and describe the same set: that is what makes
 * an item's streamed tiles and a wave's masked tiles two array reads (csrc/usp_tile_range.h), and it holds for documents laid
 * out in order.  The library cannot check it.  Arrays that break it give wrong results, never an out-of-range access: every
 * value read is clamped to [0, Sk] / [0, Sq].
 * Nothing else about the function changes: `lse` is the logsumexp over the visible keys; a row that sees no key gives out = 0,
 * lse = -inf and zero gradients, as ever.  A row tile never touches the key tiles in front of its first row's bound, and a
 * key block never the row tiles behind its last key's: eight equal documents cost about an eighth of the causal triangle.
 *   - row_lo == NULL (backward: and key_hi == NULL) is exactly usp_flash_fwd / usp_flash_bwd: the same kernels, bit-identical
 *     results, the strides ignored.  An all-zero row_lo (one document) runs the document kernels and gives the same bits as
 *     the two-waves-per-SIMD family (USP_FORCE_WAVE32);
 *   - backward: the dQ launch reads row_lo and the dK/dV launch reads key_hi.  Exactly one of them NULL is USP_EINVAL, unless
 *     USP_BWD_SKIP_* drops the launch that would read the missing one;
 *   - causal may be 0 or 1: a ring block that lies wholly below the diagonal is a full block with a left bound;
 *   - a negative stride is USP_EINVAL;
 *   - USP_ATTN_SOFTCAP, USP_ATTN_WINDOW, USP_ATTN_SHIFT, a packed batch (seq_q / seq_k) and USP_FORCE_ROW64 are
 *     USP_EUNSUPPORTED, nothing launched or written (these checks follow the argument checks every call gets, as for ALiBi);
 *   - k_splits, dq_splits and dkdv_splits are IGNORED with the arrays: the launch is served uncut and never refused for them.
 *     The workspace functions are unchanged; a workspace sized for cuts is merely not used for them (the dkdv_heads partials
 *     still are).  Cuts under a per-row bound are later work;
 *   - every head dim runs on the two-waves-per-SIMD family (document instantiations of its kernels: the forward keeps the
 *     pipelined loop for the tiles the bound cuts for no row of the item, as the window kernel does); usp_last_launch_kinds()
 *     reports the wave8 / wave4 / reduce bits that were launched.
 * Everything else is as the argument block says (dkdv_heads, merge_in, final_begin / final_end with acc, USP_LAUNCH_INTERLEAVE,
 * USP_BWD_SKIP_*, GQA, dq16 / dk16 / dv16, both 16-bit types, head dims 32 / 64 / 128, any aligned layout).  The document mask
 * together with ALiBi, dropout or sinks has no entry point.
 * -------------------------------------------------------------------------------------------- */
int usp_flash_fwd_doc(const usp_fwd_args* args, const int32_t* row_lo, int64_t row_lo_stride_b, void* stream);
int usp_flash_bwd_doc(const usp_bwd_args* args, const int32_t* row_lo, int64_t row_lo_stride_b, const int32_t* key_hi,
                      int64_t key_hi_stride_b, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Span bound: usp_flash_fwd_doc / usp_flash_bwd_doc with a right key bound read per row in place of the causal diagonal.  Inside a
 * bidirectional span (an image or prefix block of a prefix-LM, a whole document of a packed encoder) every row sees the whole
 * span; for one launch (a whole sequence, or one block of a ring) that is
 *     row i sees key j   iff   row_lo[i] <= j < row_hi[i]      ( equally:  key_lo[j] <= i < key_hi[j] ),
 * with four HOST-computed DEVICE int32 arrays in the LAUNCH'S OWN coordinates, laid out and strided like row_lo / key_hi above:
 *     row_lo[i] in [0, Sk]   the first key row i sees                        key_lo[j] in [0, Sq]   the first row that sees key j
 *     row_hi[i] in [0, Sk]   one past the last key row i sees                                         ( = #{ i : row_hi[i] <= j } )
 *                                                                            key_hi[j] in [0, Sq]   one past the last row that sees it
 *                                                                                                     ( = #{ i : row_lo[i] <= j } )
 * ALL FOUR MUST BE NON-DECREASING and describe the same set; a row is empty when row_lo[i] >= row_hi[i].  The library cannot check
 * it.  Arrays that break it give wrong results, never an out-of-range access: every value read is clamped to [0, Sk] / [0, Sq].
 * THE DIAGONAL IS FOLDED INTO row_hi BY THE CALLER (a causal row outside every span has row_hi[i] = i + 1 + Sk - Sq in a diagonal
 * block): these launches run with causal = 0.  Nothing else about the function changes: `lse` is the logsumexp over the visible
 * keys; a row or a launch that sees nothing gives out = 0, lse = -inf and zero gradients, as ever.  A row tile touches no key tile
 * in front of its first row's row_lo and none at or past ceil(row_hi[last valid row] / tile); a key block no row tile in front of
 * key_lo[first key] / tile and none behind its last key's key_hi.
 *   - row_hi == NULL (backward: and key_lo == NULL) is exactly usp_flash_fwd_doc / usp_flash_bwd_doc on the remaining arrays -- and
 *     so, with everything NULL, the plain launch: the same kernels, bit-identical results, the strides of the absent arrays ignored;
 *   - forward: with row_hi, row_lo == NULL means "all zero";
 *   - backward: the dQ launch reads (row_lo, row_hi) and the dK/dV launch (key_lo, key_hi).  With row_hi or key_lo, a launch that
 *     is not skipped and lacks one of its two arrays is USP_EINVAL; USP_BWD_SKIP_* drops the requirement for the skipped launch;
 *   - a negative stride is USP_EINVAL;
 *   - with row_hi / key_lo: causal != 0, USP_ATTN_SOFTCAP, USP_ATTN_WINDOW, USP_ATTN_SHIFT, a packed batch (seq_q / seq_k) and
 *     USP_FORCE_ROW64 are USP_EUNSUPPORTED, nothing launched or written (these checks follow the argument checks every call gets);
 *   - k_splits, dq_splits and dkdv_splits are IGNORED with the arrays, as under the document mask;
 *   - every head dim runs on the two-waves-per-SIMD family (span instantiations of its kernels: a wave's tiles below its first
 *     row's row_hi, and past its item's last row_lo, keep the pipelined loop); usp_last_launch_kinds() reports the wave8 / wave4 /
 *     reduce bits that were launched.
 * Everything else is as the argument block says (dkdv_heads, merge_in, final_begin / final_end with acc, USP_LAUNCH_INTERLEAVE,
 * USP_BWD_SKIP_*, GQA, dq16 / dk16 / dv16, both 16-bit types, head dims 32 / 64 / 128, any aligned layout).  Spans together
 * with ALiBi, dropout or sinks have no entry point.
 * -------------------------------------------------------------------------------------------- */
int usp_flash_fwd_span(const usp_fwd_args* args, const int32_t* row_lo, int64_t row_lo_stride_b, const int32_t* row_hi,
                       int64_t row_hi_stride_b, void* stream);
int usp_flash_bwd_span(const usp_bwd_args* args, const int32_t* row_lo, int64_t row_lo_stride_b, const int32_t* row_hi,
                       int64_t row_hi_stride_b, const int32_t* key_lo, int64_t key_lo_stride_b, const int32_t* key_hi,
                       int64_t key_hi_stride_b, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Block-sparse mask: usp_flash_fwd / usp_flash_bwd with a set of visible 128 x 128 blocks per (batch, query head).  Selected-block
 * attention (MoBA, NSA), block-sparse video attention: a row block sees a non-contiguous set of key blocks, often chosen on the
 * device at every step.  For one launch (a whole sequence, or one block of a ring; Sq == Sk) that is
 *     row i sees key j   iff   mask[b][h][i / 128][j / 128] != 0   and   the mask of the argument block (causal, ragged Sk) lets it,
 * with `mask` a DEVICE array of bytes (0 = hidden), block (r, c) of head h of batch b at
 *     mask[b * mask_stride_b + h * mask_stride_h + r * mask_stride_row + c],     r, c in [0, ceil(Sq / USP_BLOCK_MASK_SIZE)),
 * strides in bytes, 0 allowed (one mask for every batch entry / every head).  h is the QUERY head.  Nothing on the call path reads
 * the mask on the host: it may be written by a kernel earlier on the same stream.  With causal != 0 set bytes above the diagonal
 * are ignored and the diagonal blocks are masked causally.  `lse` is the logsumexp over the visible keys; a row that sees nothing
 * gives out = 0, lse = -inf and zero gradients, as ever.
 * `lists` is DEVICE scratch of usp_block_list_bytes(B, Hq, nb, nb) bytes (nb = ceil(Sq / 128)), 4-byte aligned, owned by the call
 * until its launches have finished: a builder launch (HBM-bound, one wave per list, no atomics) compacts the mask into int32 lists
 * [count, ascending tile indices] at the kernels' 64-wide tile granularity -- per (b, h, row block) for the forward, per
 * (b, h, pair of row blocks) with one "live" bit per half for dQ, and the transpose per (b, h, key block) for dK/dV; under causal
 * without the blocks above the diagonal -- and the kernels stream the listed tiles only.  The forward builds and reads the first
 * family, the backward the other two (of the launches USP_BWD_SKIP_* leaves).  Every count and entry is clamped as read: a
 * corrupt workspace gives wrong results, never an out-of-range access.
 *   - mask == NULL is exactly usp_flash_fwd / usp_flash_bwd: the same kernels, bit-identical results, strides and lists ignored.
 *     An all-set mask runs the block-sparse kernels and gives the bits of the two-waves-per-SIMD family's launch of the same
 *     workgroup shape (forward: the 4-wave, 128-row shape);
 *   - a negative stride, and lists == NULL or not 4-byte aligned, are USP_EINVAL;
 *   - USP_ATTN_SOFTCAP, USP_ATTN_WINDOW, USP_ATTN_SHIFT, a packed batch (seq_q / seq_k), USP_FORCE_ROW64 and Sq != Sk are
 *     USP_EUNSUPPORTED, nothing launched or written (these checks follow the argument checks every call gets);
 *   - k_splits, dq_splits and dkdv_splits are IGNORED with the mask, as under the document mask;
 *   - every head dim runs on the two-waves-per-SIMD family (block-sparse instantiations of its kernels; the forward always in the
 *     4-wave shape, whose work item is one mask row block: the listed tiles below a wave's diagonal keep the pipelined loop);
 *     usp_last_launch_kinds() reports what was launched: fwd_wave4 for the forward, the wave8 / reduce bits for the backward.
 * Everything else is as the argument block says (dkdv_heads -- each query head of a dK/dV item streams its own list --, merge_in,
 * final_begin / final_end with acc, USP_LAUNCH_INTERLEAVE, USP_BWD_SKIP_*, GQA, dq16 / dk16 / dv16, both 16-bit types, head dims
 * 32 / 64 / 128, any aligned layout).  The block mask together with ALiBi, dropout, sinks, documents or spans has no entry point.
 * -------------------------------------------------------------------------------------------- */
#define USP_BLOCK_MASK_SIZE 128
int64_t usp_block_list_bytes(int32_t B, int32_t Hq, int32_t n_row_blocks, int32_t n_key_blocks);
/* The builder launch alone, on `stream`: the lists of `which` (1: forward, 2: dQ, 4: dK/dV; any sum) of an S x S launch, exactly as
 * the two entry points below build them into `lists` (tools and tests time it and read the lists back; a call of the entry
 * points needs no call of this).  USP_EINVAL: a NULL or misaligned pointer, a non-positive size, a negative stride, which outside 1..7. */
int usp_block_lists_build(const void* mask, int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_row, int32_t B, int32_t Hq,
                          int32_t S, int32_t causal, int32_t which, void* lists, void* stream);
int usp_flash_fwd_bsp(const usp_fwd_args* args, const void* mask, int64_t mask_stride_b, int64_t mask_stride_h,
                      int64_t mask_stride_row, void* lists, void* stream);
int usp_flash_bwd_bsp(const usp_bwd_args* args, const void* mask, int64_t mask_stride_b, int64_t mask_stride_h,
                      int64_t mask_stride_row, void* lists, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Top-k block selection: the producer of a block mask for usp_flash_fwd_bsp / usp_flash_bwd_bsp, on the same stream.  The MoBA
 * gate at the kernels' block size: with nb = ceil(S / USP_BLOCK_MASK_SIZE), G = Hq / Hkv,
 *     qbar[b][I][h] = fp32 mean of the rows of block I of q (a ragged last block: over the rows it has), kbar likewise,
 *     score[b][h][I][J] = scale * qbar[b][I][h] . kbar[b][J][h / G],
 * row block I (global index Ig = row_block0 + I) sees the candidates J < nbk, under causal J <= Ig; the FORCED blocks
 * J < keep_first and Ig - keep_local < J <= Ig (of the visible ones) are always selected, and beside them the best
 * max(0, top_k - n_forced) of the other visible candidates, by score descending, ties to the lower J: exactly
 * min(max(top_k, n_forced), n_visible) bytes of a row are set.  EVERY byte of the mask is written (0 or 1), the ones above the
 * diagonal included.  Nothing is read on the host, there are no atomics, and results leave in ordinary vector stores.  With NaN
 * or infinite inputs the selection is unspecified; every access stays in range.
 *
 * usp_block_means pools a 16-bit (B, S, H, D) tensor `x` (strides in elements, head dim contiguous) into `out`, fp32
 * (B, nb, H, D) contiguous.  HBM-bound: every element is read once, in 16-byte loads.  A block's 128 rows are added in 8 runs of
 * 16 rows, each in ascending row order, and the runs in ascending order: the order of every sum is a function of (row, d) alone,
 * so the result does not depend on B, H, the grid or the workgroup that holds a block.  The last block is divided by its own row
 * count.  D: any multiple of 8 up to 128.
 *   - a NULL pointer, a non-positive size, a negative stride or a dtype other than USP_BF16 / USP_FP16 is USP_EINVAL;
 *   - another D, `x` off a 16-byte boundary or a stride that is no multiple of 8 elements is USP_EUNSUPPORTED.
 *
 * usp_block_select takes the means -- qbar fp32 (B, nbq, Hq, D), kbar fp32 (B, nbk, Hkv, D), both contiguous and 16-byte aligned
 * -- and writes mask[b * mask_stride_b + h * mask_stride_h + I * mask_stride_row + J] for I < nbq, J < nbk (strides in bytes, h the
 * QUERY head).  On one device nbq = nbk = nb and row_block0 = 0; rank r of a ring of n-block slices pools its own slices,
 * gathers kbar over the ring and selects its nbq = n rows against all nbk = nb key blocks with row_block0 = r * n.  One
 * workgroup per (b, h, I): the scores in fp32 (one chain of fused multiply-adds over ascending d), the k-th largest found exactly
 * on order-preserving integer keys in LDS, ties by a prefix over ascending J.
 *   - a NULL pointer, a non-positive size, a negative row_block0 / top_k / keep_first / keep_local / stride, a NaN scale, and
 *     causal != 0 with keep_local < 1 (a row must keep its own block) are USP_EINVAL;
 *   - D not a multiple of 8 or above 128, Hq % Hkv != 0, qbar / kbar off a 16-byte boundary and nbk > USP_BLOCK_SELECT_MAX_BLOCKS
 *     (8192 blocks = 1M tokens: the keys of one row live in LDS) are USP_EUNSUPPORTED; nothing is launched or written.
 * -------------------------------------------------------------------------------------------- */
#define USP_BLOCK_SELECT_MAX_BLOCKS 8192
int usp_block_means(const void* x, int32_t dtype, int32_t B, int32_t S, int32_t H, int32_t D, int64_t stride_b, int64_t stride_s,
                    int64_t stride_h, float* out, void* stream);
int usp_block_select(const float* qbar, const float* kbar, int32_t B, int32_t Hq, int32_t Hkv, int32_t D, int32_t nbq, int32_t nbk,
                     int32_t row_block0, float scale, int32_t causal, int32_t top_k, int32_t keep_first, int32_t keep_local,
                     void* mask, int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_row, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Top-p block selection: usp_block_select with a cumulative-mass rule in place of the count (FlexPrefill, XAttention, SpargeAttn,
 * Twilight: the fewest key blocks whose softmax mass reaches top_p).  qbar, kbar, score, Ig, the visible and the FORCED blocks,
 * the mask layout and the ring use (nbq rows from row_block0 against all nbk key blocks) are those of usp_block_select above.
 * For one (b, h, I), in real numbers:
 *     w[J] = exp(score[J] - m) / Z over the VISIBLE blocks (m their maximum, Z their sum; the forced ones included), 0 elsewhere;
 *     the forced blocks are selected, and their mass counts;
 *     the other visible blocks are ordered by w descending, ties to the lower J, and the SHORTEST prefix of that order with
 *     mass(forced) + mass(prefix) >= top_p is selected beside them (none where the forced blocks alone reach top_p; with
 *     top_p = 1 blocks whose weight has underflowed to zero may be left out).
 * share_group != 0: w[J] is the mean over the G = Hq / Hkv query heads of KV head h / G of their per-head weights -- each head
 * normalised by its own Z, not a softmax of averaged scores -- and all G heads get the same mask row (NSA's rule).  With G = 1
 * the result is bit for bit the unshared one.  EVERY byte of the mask is written (0 or 1).  Nothing is read on the host, there
 * are no atomics, results leave in ordinary vector stores.  With NaN or infinite inputs the selection is unspecified; every
 * access stays in range.
 *
 * In fp32, one workgroup of 256 threads per (b, h, I) -- share_group: per (b, KV head, I), the group's heads in ascending order:
 *   - score[J]: one chain of fused multiply-adds over ascending d from 0, times scale; m: the maximum (exact);
 *     e[J] = expf(score[J] - m); Z = SUM(e); W[J] = e[J] / Z, with share_group W[J] = (..(e0[J] / Z0 + e1[J] / Z1) + ..), the SUM
 *     over the heads (not divided by G: the rule compares against top_p * total);
 *   - SUM(x), the one order of every sum over blocks: thread t adds x[t], x[t + 256], ... ascending from 0; the 64 lanes of a
 *     wave are added by the butterfly x += x[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; the four waves ((w0 + w1) + w2) + w3.  A sum
 *     over a subset is SUM with 0 for the blocks left out: the order is a function of J alone, so results do not depend on the
 *     grid and repeat from call to call, and with non-negative terms the sum is monotone in the subset;
 *   - total = SUM(W), target = top_p * total (one fp32 product); key[J] = the order-preserving integer of W[J];
 *     mass(T) = SUM(W[J] where J is forced, or a non-forced visible block with key[J] >= T);
 *     the cut T = the largest 32-bit T with mass(T) >= target, found bit by bit from the top bit down;
 *   - selected: the forced blocks, the non-forced visible blocks with key > T, and of those with key == T (n_eq blocks of the
 *     one weight wt) the first `need` in ascending J, where with m_gt = mass(T + 1)
 *         need = the smallest c in [1, n_eq] with fmaf((float)c, wt, m_gt) >= target, n_eq where no c has
 *     (one fused multiply-add and one comparison per count; fmaf is monotone in c).
 *   - the argument rules of usp_block_select; besides, a top_p that is NaN, <= 0 or > 1 is USP_EINVAL;
 *   - USP_EUNSUPPORTED as for usp_block_select (D, Hq % Hkv, alignment, nbk > USP_BLOCK_SELECT_MAX_BLOCKS: the weights and
 *     a scratch row live in LDS, 64 KiB + 544 bytes at the limit); nothing is launched or written.
 * -------------------------------------------------------------------------------------------- */
int usp_block_select_top_p(const float* qbar, const float* kbar, int32_t B, int32_t Hq, int32_t Hkv, int32_t D, int32_t nbq,
                           int32_t nbk, int32_t row_block0, float scale, int32_t causal, float top_p, int32_t keep_first,
                           int32_t keep_local, int32_t share_group, void* mask, int64_t mask_stride_b, int64_t mask_stride_h,
                           int64_t mask_stride_row, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Block attention mass: the block-pooled attention map, the quantity the block gates above approximate (the recall of a block
 * mask is the mass on its selected blocks; SeerAttention distils its gate from this map).  q is 16-bit (B, Sq, Hq, D), k 16-bit
 * (B, Sk, Hkv, D), both with strides in elements and the head dim contiguous; lse is fp32 with lse[b * lse_stride_b +
 * h * lse_stride_h + i] the log-sum-exp of row i (natural log, of the scaled scores: what usp_flash_fwd writes).  With
 * G = Hq / Hkv, nbq = ceil(Sq / USP_BLOCK_MASK_SIZE), nbk = ceil(Sk / USP_BLOCK_MASK_SIZE), in real numbers:
 *     mass[b][h][I][J] = (1 / rows(I)) * sum over the rows i of block I (i < Sq) and the keys j of block J VISIBLE to i of
 *                        exp(scale * q[b][i][h] . k[b][j][h / G] - lse[b][h][i]),
 * where every key j < Sk is visible, under causal != 0 only j <= i + diag, and rows(I) is the number of rows block I has (a
 * ragged last block counts the rows it has: the rule of usp_block_means).  A row with lse = -inf contributes 0.  With the lse of
 * the same attention call every row of mass sums to 1 over J (under sinks: to 1 minus the sink's share).  out[b * out_stride_b +
 * h * out_stride_h + I * out_stride_row + J] is written for EVERY I < nbq, J < nbk (strides in elements: a caller may point it at
 * a column slice of a larger result), blocks above the diagonal as 0.  fp32, no atomics, ordinary vector stores, nothing read on
 * the host.  With NaN inputs or a +inf lse the result is unspecified; every access stays in range.
 *
 * One work item per (b, h, I) walks the 64-key tiles up to the item's last visible key: S^T = K Q^T on v_mfma_f32_32x32x16, one
 * chain over ascending d per score, then p = exp2(fma(s, c, -(lse_i * log2e))) with c = scale * log2e (one fp32 product each; exp2 is
 * v_exp_f32), a hidden key's p set to 0.  ORDER of the sum of one (I, J), a function of the position inside the block alone:
 *   1. the lane of (row i = 32 w + l, half hf) adds ascending from 0.f its 64 keys: the tile of keys 128 J .. + 63, then the tile
 *      128 J + 64 .. + 127; inside a tile at kt0 the keys kt0 + 4 hf + (r & 3) + 8 (r >> 2), r = 0 .. 15, then those + 32, r = 0 .. 15;
 *   2. the two halves of a row: x(hf = 0) + x(hf = 1);
 *   3. the 32 rows l of wave w by the butterfly x += x[l ^ 16], ^ 8, ^ 4, ^ 2, ^ 1;
 *   4. the four waves ((w0 + w1) + w2) + w3;   5. one division by rows(I).
 * Terms left out (hidden keys, rows past Sq, tiles the item does not reach) enter as +0.  So the result repeats from call to
 * call and does not depend on the grid, B or H; a launch on the rows [r n, (r + 1) n) against the keys [c n, (c + 1) n), n a
 * multiple of 128, with diag = (r - c) * n gives bit for bit the corresponding sub-matrix of the whole call (a ring's step).
 *   - a NULL pointer, a non-positive size, a negative stride, a dtype other than USP_BF16 / USP_FP16 or a NaN scale is USP_EINVAL;
 *   - D other than 32 / 64 / 128, Hq % Hkv != 0, q / k off a 16-byte boundary or with a stride that is no multiple of 8 elements,
 *     lse / out off a 4-byte boundary, Sq, Sk or |diag| >= 2^29 and a k row stride of 2^24 elements or more are
 *     USP_EUNSUPPORTED; nothing is launched or written.
 * -------------------------------------------------------------------------------------------- */
int usp_block_attn_mass(const void* q, const void* k, const float* lse, int32_t dtype, int32_t B, int32_t Sq, int32_t Sk, int32_t Hq,
                        int32_t Hkv, int32_t D, int64_t q_stride_b, int64_t q_stride_s, int64_t q_stride_h, int64_t k_stride_b,
                        int64_t k_stride_s, int64_t k_stride_h, int64_t lse_stride_b, int64_t lse_stride_h, float scale,
                        int32_t causal, int32_t diag, float* out, int64_t out_stride_b, int64_t out_stride_h, int64_t out_stride_row,
                        void* stream);

/* Bytes of scratch with which the backward launches get more, smaller work items (fp32 partials + one deterministic,
 * HBM-bound reduce launch each; results identical up to fp32 summation order):
 *   - GQA (Hq > Hkv): a dK/dV work item streams dkdv_heads query heads of its KV group (ABI v7; rounds 1-5: one or all).
 *     With fewer than Hq/Hkv heads per item there are (Hq/Hkv)/dkdv_heads times more items -- what balances the causal
 *     triangle when B*Hkv*ceil(Sk/128) is small -- and as many fp32 partial slabs.  dkdv_heads = 0: the largest divisor of
 *     Hq/Hkv up to 2 that leaves two work items per CU for causal / windowed launches (more heads per item let the concurrent
 *     workgroups' Q / dO streams drift out of one L2), up to 4 and one item per CU for full ones -- measured:
 *     profiles/r06_gqa_loop.txt; packed batches: 1;
 *   - dkdv_splits = n (ABI v5): every such item is cut into n items over equal runs of the query tiles that see its keys;
 *   - dq_splits = n (ABI v5): every (head, 256-row query block) item of the dQ launch is cut into n items over equal runs
 *     of the key tiles it sees -- for launches with few heads (a small head group, a high Ulysses degree), where a causal
 *     launch otherwise lasts as long as its heaviest item.
 * = 2 * ((Hq/Hkv)/dkdv_heads) * max(1, dkdv_splits) * rows_k * Hkv * D * 4  (0 when that is a single slab)
 *   + dq_splits * B * Sq * Hq * D * 4                           (0 when dq_splits <= 1); the cuts are ignored for packed
 * batches.  Passing less (or NULL) is valid and selects the whole group per work item without cuts. */
int64_t usp_flash_bwd_workspace_bytes(const usp_bwd_args* args);

/* delta[b,h,s] = sum_d dout[b,s,h,d] * out[b,s,h,d]   (fp32; delta is (B,H,S), seq stride 1).
 * The "softmax_d" term flash-attn's backward derives from `out` (its 5th positional argument,
 * kernels/attention.py:205). */
int usp_bwd_delta(int32_t dtype, int32_t B, int32_t S, int32_t H, int32_t D,
                  const usp_tensor* dout, const usp_tensor* out,
                  float* delta, int64_t delta_stride_b, int64_t delta_stride_h, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Stand-alone LSE merge: update_out_and_lse (yunchang/ring/utils.py:10-51) as one kernel.
 *   acc (B,S,H,D) fp32, lse (B,H,S) fp32 are updated in place with a block result
 *   blk_out (B,S,H,D) 16-bit, blk_lse (B,H,S) fp32.  first != 0: adopt the block (utils.py:38-42).
 * -------------------------------------------------------------------------------------------- */
int usp_lse_merge(int32_t dtype, int32_t B, int32_t S, int32_t H, int32_t D,
                  const usp_tensor* acc, float* lse, int64_t lse_stride_b, int64_t lse_stride_h,
                  const usp_tensor* blk_out, const float* blk_lse, int64_t blk_lse_stride_b,
                  int64_t blk_lse_stride_h, int32_t first, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Row-gather copy used to build / unpack the Ulysses all-to-all buffers
 * (the two `.contiguous()` transposes of yunchang/comm/all_to_all.py:39-49,62-65,76-84,98-100).
 *   for i0<n0, i1<n1, i2<n2, i3<n3:
 *     dst[i0*ds0 + i1*ds1 + i2*ds2 + i3*ds3 + (0..row_bytes)] = src[i0*ss0 + ... ]
 * Strides in BYTES; row_bytes, all strides and both pointers must be multiples of 16.
 * -------------------------------------------------------------------------------------------- */
int usp_copy_rows(void* dst, const void* src, int64_t row_bytes,
                  int64_t n0, int64_t n1, int64_t n2, int64_t n3,
                  int64_t ds0, int64_t ds1, int64_t ds2, int64_t ds3,
                  int64_t ss0, int64_t ss1, int64_t ss2, int64_t ss3, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Row-gather with an r-term sum: the dK/dV return of a Ulysses exchange whose KV heads are shared by
 * r = P / Hkv ranks (each rank sends its partial sum over its own query heads; the owner adds them).
 *   for i0<n0, i1<n1, i2<n2:
 *     dst[i0*ds0 + i1*ds1 + i2*ds2 + (0..row_bytes)] =
 *         round( sum_{t=0..r-1} src[t*term_stride + i0*ss0 + i1*ss1 + i2*ss2 + (0..row_bytes)] )
 * Elements of `dtype` (USP_BF16 / USP_FP16), accumulated in fp32 in ascending t and rounded once.
 * Strides in BYTES; row_bytes, term_stride, all strides and both pointers must be multiples of 16
 * (USP_EUNSUPPORTED); null pointers, r < 1 or non-positive sizes are USP_EINVAL.
 * -------------------------------------------------------------------------------------------- */
int usp_sum_rows(int32_t dtype, void* dst, const void* src, int64_t row_bytes, int32_t r, int64_t term_stride,
                 int64_t n0, int64_t n1, int64_t n2, int64_t ds0, int64_t ds1, int64_t ds2,
                 int64_t ss0, int64_t ss1, int64_t ss2, void* stream);

/* dst16[i] = round(src32[i]) for i < n, `rows` rows of `n` contiguous elements with row strides
 * (elements) -- the `.to(q.dtype)` casts at zigzag_ring_flash_attn.py:74,183. */
int usp_cast_from_f32(int32_t dtype, void* dst, int64_t dst_row_stride, const float* src,
                      int64_t src_row_stride, int64_t rows, int64_t n, void* stream);

/* dst[r, i] = a[r, i] + b[r, i]  (fp32; any of the three may alias) -- the dk/dv accumulator adds
 * at zigzag_ring_flash_attn.py:161-170 / ring_flash_attn.py:130-131. */
int usp_add_f32(float* dst, int64_t dst_row_stride, const float* a, int64_t a_row_stride,
                const float* b, int64_t b_row_stride, int64_t rows, int64_t n, void* stream);

/* What the LAST usp_flash_fwd / usp_flash_bwd call of the CALLING THREAD launched: a mask of USP_KIND_* bits (0 before
 * the first call and after a call that returned an error before launching).  Thread-local: no state is shared between
 * threads, the entry points stay re-entrant.  For tests ("assert the 64-row forward ran") and bench labels. */
enum {
  USP_KIND_FWD_ROW64 = 1,       /* flash_fwd64_kernel        (4 waves x 64 rows) */
  USP_KIND_FWD_WAVE8 = 2,       /* flash_fwd_kernel, 8 waves (256 rows per item) */
  USP_KIND_FWD_WAVE4 = 4,       /* flash_fwd_kernel, 4 waves (128 rows per item) */
  USP_KIND_FWD_SPLIT_MERGE = 8, /* split_merge_kernel behind a K-split launch */
  USP_KIND_DKDV_ROW64 = 16,     /* flash_bwd_dkdv64_kernel */
  USP_KIND_DKDV_WAVE8 = 32,     /* flash_bwd_dkdv_kernel */
  USP_KIND_DQ_ROW64 = 64,       /* flash_bwd_dq64_kernel */
  USP_KIND_DQ_WAVE8 = 128,      /* flash_bwd_kernel (dQ) */
  USP_KIND_REDUCE_HEADS = 256,  /* reduce_heads_kernel (GQA head split / dK,dV cuts) */
  USP_KIND_REDUCE_CUTS = 512,   /* reduce_cuts_kernel (dQ key cuts) */
  USP_KIND_DKDV_KEYS256 = 1024  /* beside USP_KIND_DKDV_ROW64: it was flash_bwd_dkdv64u_kernel (256-key items) */
};
int usp_last_launch_kinds(void);

/* Diagnostic (ABI v6), not a replacement of any reference call site: what the matrix pipe of THIS part sustains on the
 * caller's operands -- an MFMA-only loop (v_mfma_f32_32x32x16_bf16, no LDS / VALU / memory traffic inside) on one workgroup
 * per CU, `waves_per_simd` (1 | 2) waves per SIMD, `iters` passes of 64 MFMAs per wave.  `operands`: >= 64 KiB of device
 * memory holding bf16 values (N(0,1) as the bench's inputs, or zeros: the part clocks by power and MFMA power depends on
 * the operand bit patterns).  FLOPs of a launch = CUs * 4 * waves_per_simd * iters * 64 * 32768.  `sink`: >= 512 floats of
 * device scratch.  `clocks` (optional, 2 x uint64 device): elapsed s_memtime (shader clock) and s_memrealtime (100 MHz)
 * ticks of one wave's loop -> sustained clock.  bench.py reports a flash kernel's rate against this ceiling beside its
 * fraction of the nominal 2.5 PFLOP/s. */
int usp_mfma_probe(const void* operands, int64_t operand_bytes, int32_t iters, int32_t waves_per_simd,
                   float* sink, uint64_t* clocks, void* stream);

int usp_abi_version(void);
/* The USP_ATTN_* bits this library serves (USP_ATTN_WINDOW | USP_ATTN_SOFTCAP | USP_ATTN_SHIFT | USP_ATTN_ALIBI |
 * USP_ATTN_DROPOUT | USP_ATTN_SINK | USP_ATTN_DOC | USP_ATTN_SPAN | USP_ATTN_BLOCK_MASK | USP_ATTN_MAX_LOGIT | USP_ATTN_BLOCK_SELECT |
 * USP_ATTN_BLOCK_SELECT_TOP_P | USP_ATTN_BLOCK_MASS, the last ten feature bits: the *_alibi / *_dropout / *_sink / *_doc / *_span /
 * *_bsp / *_maxlogit / usp_block_means and usp_block_select / usp_block_select_top_p / usp_block_attn_mass entry points exist).
 * Unknown flag bits are not rejected by usp_flash_fwd / usp_flash_bwd, so a binding checks here before it relies on a bit added after ABI v7's first release. */
int usp_attn_features(void);
const char* usp_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif /* USP_HIP_H */
