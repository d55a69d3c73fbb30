"""Block attention kernels of the USP path, backed by libusp_hip.so.

Mirrors the callables yunchang/kernels/attention.py exposes to the ring schedules:
  * hip_attn_forward  <->  pytorch_attn_forward(op_type="efficient") (attention.py:44-136) /
                           flash_attn_forward (:165-202)            [the `fwd-only` contract]
  * hip_attn_backward <->  flash_attn_backward (:205-250)           [the `bwd-only` contract;
                           pytorch_attn_backward (:138-159) raises in the reference]
and defines the richer internal seam (`BlockBackend`) the ring schedules of THIS package use, in
which the LSE merge (ring/utils.py:10-51) and the fp32 gradient accumulation
(zigzag_ring_flash_attn.py:147-170) are fused into the kernels.
"""
from __future__ import annotations

import torch

from .. import _C
from .features import (BLOCK_MASK_SIZE, BlockSelect, BlockSelectTopP, Features, block_mask_alone, block_mask_self_attention,  # noqa: F401
                       block_select_alone, expand_block_mask, max_logits_alone, return_block_mass_alone)


def kernel_operand(t: torch.Tensor) -> torch.Tensor:
    """A tensor autograd hands to a backward as-is may be anything -- `out.sum().backward()` delivers an EXPANDED scalar
    (every stride 0), a slice of a bigger gradient has odd strides.  The kernels want unit head-dim stride and 16-byte
    multiples elsewhere (flash-attn's `maybe_contiguous`, flash_attn_interface.py, does the same for the reference)."""
    if t.is_contiguous() and t.storage_offset() == 0:       # the common case, one C++ call
        return t
    es = t.element_size()
    ok = t.stride(-1) == 1 and all(t.shape[d] == 1 or (t.stride(d) * es) % 16 == 0 for d in range(t.dim() - 1)) \
        and (t.storage_offset() * es) % 16 == 0
    return t if ok else t.contiguous()


KERNEL_HEAD_DIMS = (32, 64, 128)      # what libusp_hip.so instantiates (include/usp_hip.h: anything else is USP_EUNSUPPORTED)


def kernel_head_dim(D: int) -> int:
    """The head dim the kernels run a `D`-dim problem at: the smallest instantiated one that holds it.  Zero-padding the head
    dim changes neither the scores (the pad contributes 0 to every dot product; the softmax scale stays D ** -0.5) nor the first D
    output dims, so head dims such as 40, 72, 80, 96, 112 -- which flash-attn serves (kernels/attention.py:177-202: any
    multiple of 8 up to 256) -- run through the entry points of this package on padded copies, at the padded dim's cost.
    Above 128 there is no kernel (a 256-dim tile does not fit the 256-register budget of the 8-wave shape)."""
    for d in KERNEL_HEAD_DIMS:
        if D <= d:
            return d
    raise NotImplementedError(f"head_dim {D} > {KERNEL_HEAD_DIMS[-1]} is not supported by the HIP attention kernels")


def pad_head_dim(*tensors):
    """Zero-pad the last dim of each tensor to kernel_head_dim (autograd-aware: torch.nn.functional.pad)."""
    D = tensors[0].shape[-1]
    Dp = kernel_head_dim(D)
    if Dp == D:
        return tensors
    return tuple(torch.nn.functional.pad(t, (0, Dp - D)) for t in tensors)


def needs_grad(*tensors) -> bool:
    """Does autograd have to record this call?  (The ring functions skip their autograd.Function otherwise.)"""
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


class HipBlockBackend:
    """The device backend: thin adapter over the C ABI (include/usp_hip.h).  Immutable: `interleave` is fixed
    at construction, so concurrent callers (the autograd thread running one layer's backward while the main
    thread runs another layer's forward) cannot disturb each other's launch mode."""

    name = "hip"

    def __init__(self, interleave: bool = False):
        # True: every flash launch carries USP_LAUNCH_INTERLEAVE (include/usp_hip.h) so that RCCL's kernels can
        # become resident beside it; False: persistent launches (fastest when the GPU does nothing else).
        self.interleave = bool(interleave)
        self._beside = self if interleave else None

    def beside_transfers(self) -> "HipBlockBackend":
        """The same backend for launches that are meant to run beside transfers on other streams (ring
        degree > 1, pipelined Ulysses exchange)."""
        if self._beside is None:
            self._beside = HipBlockBackend(interleave=True)
        return self._beside

    def fwd(self, q, k, v, softmax_scale, causal, lse, out=None, acc=None, merge_in=False,
            final_begin=0, final_end=None, window=None, k_splits=None, softcap=None, shift=None, alibi=None, dropout=None,
            sinks=None, doc=None, span=None, bsp=None, row_max=None):
        _C.flash_fwd(q, k, v, softmax_scale, causal, lse, out, acc, merge_in, final_begin, final_end,
                     interleave=self.interleave, window=window, k_splits=k_splits, softcap=softcap, shift=shift, alibi=alibi,
                     dropout=dropout, sinks=sinks, doc=doc, span=span, bsp=bsp, row_max=row_max)

    def row_max_reduce(self, row_max, out=None, accum=False):
        """(Hq,) fp32: the maximum over batch and rows of the (B, Hq, S) row maxima a `row_max=` forward left (no host read)."""
        return _C.row_max_reduce(row_max, out=out, accum=accum)

    def sink_grad(self, sinks, lse, delta, out=None, accum=False):
        return _C.sink_grad(sinks, lse, delta, out=out, accum=accum)

    def block_means(self, x):
        """fp32 (B, nb, H, D): the means of the 128-row blocks of a 16-bit (B, S, H, D) operand (usp_block_means)."""
        return _C.block_means(x)

    def block_select(self, qbar, kbar, top_k, scale, causal, keep_first=0, keep_local=1, row_block0=0):
        """torch.bool (B, Hq, nbq, nbk): the selected key blocks of the row blocks whose means are `qbar`, the first of them the
        global row block `row_block0`, among the key blocks whose means are `kbar` (usp_block_select; no host read)."""
        return _C.block_select(qbar, kbar, top_k, scale, causal, keep_first, keep_local, row_block0)

    def block_select_top_p(self, qbar, kbar, top_p, scale, causal, keep_first=0, keep_local=1, share_group=False, row_block0=0):
        """torch.bool (B, Hq, nbq, nbk): block_select's mask by cumulative softmax mass (usp_block_select_top_p; no host read)."""
        return _C.block_select_top_p(qbar, kbar, top_p, scale, causal, keep_first, keep_local, share_group, row_block0)

    def block_mass(self, q, k, lse, scale, causal, diag=0, out=None):
        """fp32 (B, Hq, nbq, nbk): the share of the softmax mass the rows of every 128-row block of q give to every 128-key block
        of k, from the rows' `lse`; under `causal` row i sees key j iff j <= i + diag; `out` may be a column slice of a larger
        result (usp_block_attn_mass; no host read)."""
        return _C.block_attn_mass(q, k, lse, scale, causal, diag, out)

    def delta(self, dout, out, delta):
        _C.bwd_delta(dout, out, delta)

    def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale, causal, accum_dq=False,
            accum_dk=False, accum_dv=False, dq16=None, dk16=None, dv16=None, window=None, only=None, softcap=None,
            shift=None, alibi=None, dropout=None, doc=None, span=None, bsp=None):
        _C.flash_bwd(dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale, causal, accum_dq,
                     accum_dk, accum_dv, dq16, dk16, dv16, interleave=self.interleave, window=window, only=only,
                     softcap=softcap, shift=shift, alibi=alibi, dropout=dropout, doc=doc, span=span, bsp=bsp)

    def fwd_packed(self, q, k, v, seq_q, seq_k, max_q, max_k, softmax_scale, causal, lse, out=None,
                   acc=None, merge_in=False, final_begin=0, final_end=2, softcap=None):
        _C.flash_fwd_packed(q, k, v, seq_q, seq_k, max_q, max_k, softmax_scale, causal, lse, out, acc,
                            merge_in, final_begin, final_end, interleave=self.interleave, softcap=softcap)

    def bwd_packed(self, dout, q, k, v, lse, delta, seq_q, seq_k, max_q, max_k, dq, dk, dv,
                   softmax_scale, causal, accum_dq=False, accum_dk=False, accum_dv=False, dq16=None,
                   dk16=None, dv16=None, softcap=None):
        _C.flash_bwd_packed(dout, q, k, v, lse, delta, seq_q, seq_k, max_q, max_k, dq, dk, dv,
                            softmax_scale, causal, accum_dq, accum_dk, accum_dv, dq16, dk16, dv16,
                            interleave=self.interleave, softcap=softcap)

    def merge(self, acc, lse, blk_out, blk_lse, first):
        _C.lse_merge(acc, lse, blk_out, blk_lse, first)

    def cast(self, dst16, src32):
        _C.cast_from_f32(dst16, src32)

    def add(self, dst, a, b):
        _C.add_f32(dst, a, b)

    def copy_rows(self, dst, src, row_bytes, sizes, dst_strides, src_strides):
        _C.copy_rows(dst, src, row_bytes, sizes, dst_strides, src_strides)

    def sum_rows(self, dst, src, row_bytes, r, term_stride, sizes, dst_strides, src_strides):
        _C.sum_rows(dst, src, row_bytes, r, term_stride, sizes, dst_strides, src_strides)


_BACKEND = HipBlockBackend()


class _FeatureBackend:
    """A block backend whose flash calls carry the keywords of the features that are on in `f` (kernels/features.py), and no
    others: a backend written before a feature existed never sees its keyword.  Everything else is the wrapped backend's.
      softcap  a per-score transform: every flash call carries `softcap=`, the packed ones too; the ring schedules, LSE merges and
               gradient folds are unchanged.
      alibi    every dense flash call carries `alibi=slopes`.  The bias of a block depends on WHERE the block lies: a caller whose
               block is not the whole sequence passes `shift=` with each call (the basic ring does, ring/ring_flash_attn.py).
      dropout  every dense flash call carries `dropout=(p, seed, row0, key0, head0)`.  The mask is a function of GLOBAL positions
               (include/usp_hip.h: usp_flash_fwd_dropout), so such a caller passes `at=(row0, key0)` -- where the block's row 0 and
               key 0 lie -- the way `shift=` is given; without it the block starts at (0, 0).
      sinks    the forward launches WITHOUT merge_in carry `sinks=`: the sink is position-free and counts once per row, so it rides
               on the launch that opens the rows' running state (every ring opens each row range with exactly one such launch);
               the later merge_in launches, the merges and the backward kernels work unchanged on an lse that holds it
               (usp_flash_fwd_sink).  (Hq,) over the heads of the block calls; sink_grad(lse, delta) binds them.
      doc      the bound of a launch depends on WHERE the launch lies, and only the schedule knows that: fwd and bwd take the
               per-launch arrays as `doc=(row_lo, key_hi)` from the schedule (ring/doc_blocks.py) and hand them on; a launch without
               the keyword is refused, so that no block of such a call can run unmasked by oversight.  Under a plan with
               bidirectional spans the schedule hands `span=(row_lo, row_hi, key_lo, key_hi)` instead -- the document bound and
               the diagonal lie inside those arrays -- and launches with causal=False (DocCall.kw / DocCall.causal).
    The packed calls serve softcap alone and refuse the rest (Features.refuse_packed)."""

    def __init__(self, be, f: Features, seed: int = 0, head0: int = 0):
        self._be, self._f, self._seed, self._head0 = be, f, int(seed), int(head0)

    def _with(self, kw):
        f = self._f
        if f.softcap is not None:
            kw["softcap"] = f.softcap
        if f.alibi is not None:
            kw["alibi"] = f.alibi
        if f.dropout is not None:
            row0, key0 = kw.pop("at", (0, 0))
            kw["dropout"] = (f.dropout, self._seed, int(row0), int(key0), self._head0)
        if f.doc is not None and kw.get("doc") is None and kw.get("span") is None:
            raise RuntimeError("a launch under cu_doclens carries its doc=(row_lo, key_hi) arrays (ring/doc_blocks.py)")
        return kw

    def fwd(self, *args, **kw):
        if self._f.sinks is not None and not kw.get("merge_in", args[8] if len(args) > 8 else False):
            kw["sinks"] = self._f.sinks
        self._be.fwd(*args, **self._with(kw))

    def bwd(self, *args, **kw):
        self._be.bwd(*args, **self._with(kw))

    def sink_grad(self, lse, delta, out=None, accum=False):
        """The rank's share of the sinks' gradient from its rows' global lse and delta (fp32 (Hq,))."""
        return self._be.sink_grad(self._f.sinks, lse, delta, out=out, accum=accum)

    def fwd_packed(self, *args, **kw):
        self._f.refuse_packed()
        self._be.fwd_packed(*args, softcap=self._f.softcap, **kw)

    def bwd_packed(self, *args, **kw):
        self._f.refuse_packed()
        self._be.bwd_packed(*args, softcap=self._f.softcap, **kw)

    def __getattr__(self, name):
        return getattr(self._be, name)


class RowMaxBackend:
    """A block backend whose forward launches also leave the rows' largest visible logit (`row_max=`, usp_flash_fwd_maxlogit), for
    the schedules that run under return_max_logits.  The row maximum is row-local and position-free and travels wherever lse
    travels -- so it is kept in a SHADOW of the lse's storage: whatever view of its lse a schedule hands a launch (all rows, the
    zigzag ring's `rows c:`, a row piece), the launch gets the same view of the shadow.  The launch that opens a row range writes
    it (merge_in off), a merging one takes the maximum, exactly as the kernels treat lse; a merge outside the kernels (`merge`)
    combines the maxima of its two lse's likewise.  `max_logits(lse)` reduces the shadow of a whole (B, Hq, S) lse to fp32 (Hq,),
    once, at the end; nothing is read on the host.  Everything else is the wrapped backend's."""

    def __init__(self, be):
        self._be, self._shadows = be, {}

    def _shadow(self, lse):
        st = lse.untyped_storage()
        held = self._shadows.get(st.data_ptr())
        if held is None:        # (the lse is kept too: its storage cannot be freed and its address reused while the shadow lives)
            held = self._shadows[st.data_ptr()] = (torch.empty(st.nbytes() // 4, dtype=torch.float32, device=lse.device), lse)
        return held[0].as_strided(lse.shape, lse.stride(), lse.storage_offset())

    def fwd(self, q, k, v, softmax_scale, causal, lse, *args, **kw):
        self._be.fwd(q, k, v, softmax_scale, causal, lse, *args, row_max=self._shadow(lse), **kw)

    def merge(self, acc, lse, blk_out, blk_lse, first):
        self._be.merge(acc, lse, blk_out, blk_lse, first)
        mine, blk = self._shadow(lse), self._shadow(blk_lse)
        if first:
            mine.copy_(blk)
        else:
            torch.maximum(mine, blk, out=mine)

    def max_logits(self, lse):
        return self._be.row_max_reduce(self._shadow(lse))

    def __getattr__(self, name):
        return getattr(self._be, name)


def draw_seed() -> int:
    """The seed of one call with dropout: one 63-bit draw from torch's default CPU generator -- host side, no device sync,
    reproducible under torch.manual_seed, advancing with every call.  Drawn in the autograd forward, kept on ctx and reused by the
    backward.  Ranks that must agree on a mask (a ring, a Ulysses group) are seeded alike by the caller."""
    return int(torch.randint(0, (1 << 63) - 1, (1,), dtype=torch.int64).item())


def rng_state_of(rng_state):
    """`rng_state` of hip_attn_forward / hip_attn_backward -> (seed, row0, key0, head0): a bare seed is a block at (0, 0, 0)."""
    if isinstance(rng_state, (tuple, list)):
        if len(rng_state) != 4:
            raise ValueError(f"rng_state must be a seed or (seed, row0, key0, head0), got {rng_state!r}")
        return tuple(int(x) for x in rng_state)
    return int(rng_state), 0, 0, 0


def get_block_backend(beside_transfers: bool = False, softcap=None, alibi=None, dropout=None, sinks=None, doc=None):
    """The block backend; `beside_transfers=True` asks for launches that leave room for collectives queued on
    other streams (a persistent flash launch holds every CU until it ends: DESIGN.md section 5).  Test
    backends without that notion are returned as they are.  `softcap` > 0 (flash-attn's logit cap): every flash
    call of the returned backend carries it; None / 0: the backend itself, whose calls carry no softcap keyword
    (backends written before softcap existed keep working).  `alibi`: flash-attn's alibi_slopes as the block calls take them
    (an fp32 (Hq,) or (B, Hq) tensor on the operands' device, _C.alibi_value), None = off: every dense flash call carries
    them.  `dropout`: (p, seed, head0), None or p = 0 = off: every dense flash call carries p, the seed and the head offset, and
    takes `at=(row0, key0)`.  `sinks`: one logit per query head of the block calls (a (Hq,) tensor on the operands' device,
    _C.sinks_value), None = off: the forward launches that open a row range carry it and the backend offers
    sink_grad(lse, delta).  `doc`: anything but None / False = the call runs under a document mask: fwd and bwd take the
    per-launch `doc=(row_lo, key_hi)` keyword from the schedule.  What each feature does to the calls: _FeatureBackend; which
    of them go together (NotImplementedError otherwise): kernels/features.py."""
    be = _BACKEND
    if beside_transfers and hasattr(be, "beside_transfers"):
        be = be.beside_transfers()
    cap = _C.softcap_value(softcap)
    p = None if dropout is None else _C.dropout_value(dropout[0])
    if doc is False:
        doc = None
    if cap is None and alibi is None and p is None and sinks is None and doc is None:
        return be                                  # nothing on (the plain call): no record
    f = Features(None, cap, alibi, p, sinks, doc).check()
    return _FeatureBackend(be, f, *(dropout[1:3] if p is not None else ()))


def set_block_backend(backend):
    """Replace the block backend.  Exists for the CPU/gloo orchestration tests, which plug the
    CPU oracle in here (tests/oracle_backend.py); the package itself only ever installs
    HipBlockBackend and has no CPU path.  Returns the previous backend."""
    global _BACKEND
    prev, _BACKEND = _BACKEND, backend
    return prev


def _default_scale(q, softmax_scale):
    return q.shape[-1] ** (-0.5) if softmax_scale is None else softmax_scale


def _dropout_of(p, rng_state, what):
    """(p, seed, row0, key0, head0) of a block call with dropout, or None when it is off (`p`: the decoded probability).  The
    block contracts return no state, so the caller supplies it: dropout_p > 0 without `rng_state` is refused."""
    if p is None:
        return None
    if rng_state is None:
        raise NotImplementedError(f"{what} with dropout_p != 0 needs rng_state=(seed, row0, key0, head0) or a seed: the "
                                  f"contract returns no state (hip_attn_func draws and keeps one per call)")
    return (p,) + rng_state_of(rng_state)


def _block_call(f: Features, q, dr):
    """(backend, per-call keywords) of the one launch of a single-block call with the features `f` and the dropout state `dr`.
    Under a plan with spans the keywords hold `span`: the caller then launches with causal=False (the diagonal is in row_hi)."""
    be = get_block_backend(softcap=f.softcap, alibi=f.alibi, dropout=None if dr is None else (dr[0], dr[1], dr[4]),
                           sinks=f.sinks, doc=f.doc)
    kw = {"window": f.window}
    if dr is not None:
        kw["at"] = (dr[2], dr[3])
    if f.doc is not None:
        kw.update(_whole_doc(f.doc, q))
    return be, kw


def _whole_doc(docs, q):
    """The `doc=` (or, under spans, `span=`) keyword of the one launch of a single-block call."""
    from ..ring import doc_blocks
    return doc_blocks.whole_call(docs, q.shape[1], q.device).kw(0)


def window_of(window_size):
    """flash-attn's `window_size` -> (left, right) or None when it selects no window ((-1, -1), None)."""
    return _C._window(window_size)


def block_mask_of(block_mask, q, k):
    """`block_mask` of a whole single-device call on q (B, S, Hq, D) and k, checked (ValueError: shape, dtype, device;
    NotImplementedError: q and k of different lengths) and returned as given; no value of it is read."""
    block_mask_self_attention(q.shape[1], k.shape[1])
    _C.block_mask_value(block_mask, q.shape[0], q.shape[2], q.shape[1], q.device)
    return block_mask


def select_operands(q, k, softmax_scale=None):
    """(q, k, scale) as the selection kernels take them: values without gradient, any view the kernels can address
    (kernel_operand), head dims the kernels do not instantiate zero-padded -- the pad adds 0 to every score -- and the scale of
    the UNPADDED head dim where none is given."""
    if q.dim() != 4 or k.dim() != 4 or q.shape[0] != k.shape[0] or q.shape[3] != k.shape[3] or q.dtype != k.dtype:
        raise ValueError(f"block selection takes q (B, S, Hq, D) and k (B, S, Hkv, D) of one 16-bit type, got {tuple(q.shape)} "
                         f"{q.dtype} and {tuple(k.shape)} {k.dtype}")
    _C.dtype_code(q.dtype)
    if k.shape[2] <= 0 or q.shape[2] % k.shape[2]:
        raise ValueError(f"block selection needs Hq a multiple of Hkv, got {q.shape[2]} and {k.shape[2]}")
    scale = float(_default_scale(q, softmax_scale))
    with torch.no_grad():
        q, k = pad_head_dim(q.detach(), k.detach())
        return kernel_operand(q), kernel_operand(k), scale


def select_blocks(q, k, top_k, *, softmax_scale=None, causal=False, keep_first=0, keep_local=1):
    """The block mask a `block_select=BlockSelect(top_k, keep_first, keep_local)` call runs under: torch.bool (B, Hq, nb, nb),
    nb = ceil(S / 128), of q (B, S, Hq, D) and k (B, S, Hkv, D) (bf16 / fp16, any strides with a unit last one), selected on the
    device and never read on the host -- the MoBA gate at the kernels' block size.  With qbar / kbar the fp32 means of the
    128-row blocks (a ragged last block: over the rows it has) and score[b, h, I, J] = softmax_scale * qbar[b, h, I] .
    kbar[b, h // (Hq / Hkv), J] (default scale: D ** -0.5), row block I sees every J, under `causal` J <= I; the blocks J <
    keep_first and I - keep_local < J <= I of them are always selected, and beside them the best max(0, top_k - n_forced) of the
    others, by score descending, ties to the lower J: every row block selects exactly min(max(top_k, n_forced), n_visible) blocks.
    Every element of the result is written (False above the diagonal under causal).  No gradient: q and k are read as values.
    ValueError: a negative or non-int top_k / keep_first / keep_local, keep_local < 1 under causal; NotImplementedError: q and k of
    different lengths, more than 8192 blocks.  With NaN or Inf inputs the selection is unspecified."""
    top_k, keep_first, keep_local = _C.block_select_value(top_k, keep_first, keep_local, causal)
    block_mask_self_attention(q.shape[1], k.shape[1], "block_select")
    q, k, scale = select_operands(q, k, softmax_scale)
    nb = (q.shape[1] + BLOCK_MASK_SIZE - 1) // BLOCK_MASK_SIZE
    if nb > _C.BLOCK_SELECT_MAX_BLOCKS:
        raise NotImplementedError(f"block_select serves up to {_C.BLOCK_SELECT_MAX_BLOCKS} blocks of {BLOCK_MASK_SIZE} keys, got {nb}")
    be = get_block_backend()
    return be.block_select(be.block_means(q), be.block_means(k), top_k, scale, bool(causal), keep_first, keep_local, 0)


def select_blocks_top_p(q, k, top_p, *, softmax_scale=None, causal=False, keep_first=0, keep_local=1, share_group=False):
    """The block mask a `block_select=BlockSelectTopP(top_p, keep_first, keep_local, share_group)` call runs under: torch.bool
    (B, Hq, nb, nb) like select_blocks, selected on the device and never read on the host.  With the scores of select_blocks,
    w[b, h, I, J] = the softmax of row (b, h, I) over the blocks it sees (every J, under `causal` J <= I); the blocks J <
    keep_first and I - keep_local < J <= I of them are always selected and their mass counts; the others are ordered by w
    descending, ties to the lower J, and the shortest prefix with mass(forced) + mass(prefix) >= top_p is selected beside them
    (nothing where the forced blocks reach top_p; with top_p = 1 blocks whose weight has underflowed to zero may be left out).
    `share_group`: w is the mean over the query heads of one KV head of their weights (each its own softmax) and the group's
    heads get the same mask (include/usp_hip.h: usp_block_select_top_p states every sum's order and the tie expression).  No
    gradient.  ValueError: a top_p outside (0, 1], a negative or non-int keep_first / keep_local, a non-bool share_group,
    keep_local < 1 under causal; NotImplementedError: q and k of different lengths, more than 8192 blocks."""
    top_p, keep_first, keep_local, share_group = _C.block_select_top_p_value(top_p, keep_first, keep_local, share_group, causal)
    block_mask_self_attention(q.shape[1], k.shape[1], "block_select")
    q, k, scale = select_operands(q, k, softmax_scale)
    nb = (q.shape[1] + BLOCK_MASK_SIZE - 1) // BLOCK_MASK_SIZE
    if nb > _C.BLOCK_SELECT_MAX_BLOCKS:
        raise NotImplementedError(f"block_select serves up to {_C.BLOCK_SELECT_MAX_BLOCKS} blocks of {BLOCK_MASK_SIZE} keys, got {nb}")
    be = get_block_backend()
    return be.block_select_top_p(be.block_means(q), be.block_means(k), top_p, scale, bool(causal), keep_first, keep_local,
                                 share_group, 0)


def _selected(block_select, q, k, softmax_scale, causal):
    """The mask of a call under `block_select` (judged alone already): by the record's type."""
    if isinstance(block_select, BlockSelectTopP):
        return select_blocks_top_p(q, k, block_select.top_p, softmax_scale=softmax_scale, causal=causal,
                                   keep_first=block_select.keep_first, keep_local=block_select.keep_local,
                                   share_group=block_select.share_group)
    return select_blocks(q, k, block_select.top_k, softmax_scale=softmax_scale, causal=causal, keep_first=block_select.keep_first,
                         keep_local=block_select.keep_local)


def mass_operands(q, k, lse, softmax_scale=None):
    """(q, k, lse, scale) as usp_block_attn_mass takes them: select_operands' q and k, and the fp32 lse (B, Hq, S_q) with a unit
    last stride, read as a value."""
    if lse.dim() != 3 or tuple(lse.shape) != (q.shape[0], q.shape[2], q.shape[1]):
        raise ValueError(f"block attention mass takes the lse (B, Hq, S) of q (B, S, Hq, D), got {tuple(lse.shape)} beside "
                         f"{tuple(q.shape)}")
    q, k, scale = select_operands(q, k, softmax_scale)
    with torch.no_grad():
        lse = lse.detach()
        if lse.dtype != torch.float32:
            lse = lse.float()
        if lse.stride(-1) != 1:
            lse = lse.contiguous()
    return q, k, lse, scale


def block_attention_mass(q, k, lse, *, softmax_scale=None, causal=False):
    """The block-pooled attention map of a self-attention call: fp32 (B, Hq, nb, nb), nb = ceil(S / 128), of q (B, S, Hq, D), k
    (B, S, Hkv, D) (bf16 / fp16, any strides with a unit last one) and the call's `lse` (B, Hq, S) -- what
    hip_attn_func(..., return_attn_probs=True) returns.  mass[b, h, I, J] is the mean over the rows i of block I of the attention
    probability row i gives to the keys of block J: sum_j exp(softmax_scale * q_i . k_j - lse_i) over the keys j of J that i
    sees (every key, under `causal` j <= i); a ragged last block is averaged over the rows it has, a row with lse = -inf adds 0,
    blocks above the diagonal are 0 and every element is written.  With the lse of the same call every row of the map sums to 1;
    with the lse of a call with sinks, to 1 minus the sink's share -- the function takes whatever lse it is given.  It is the
    ground truth the block gates (select_blocks, select_blocks_top_p) approximate: block_mask_recall(mass, mask) is the recall of
    a mask.  Computed on the device by one kernel that forms no S x S scores in memory (include/usp_hip.h: usp_block_attn_mass
    states the order of every sum; results repeat bit for bit); never read on the host, no gradient.  Padded head dims are
    included.  NotImplementedError: q and k of different lengths."""
    block_mask_self_attention(q.shape[1], k.shape[1], "block_attention_mass")
    q, k, lse, scale = mass_operands(q, k, lse, softmax_scale)
    return get_block_backend().block_mass(q, k, lse, scale, bool(causal), 0)


def block_mask_recall(mass, mask):
    """The recall of a block mask under a block attention map: (B, Hq, nbq), the sum over J of mass * mask -- the share of the
    softmax mass of every row block that lies on the blocks the mask selects (the figure the FlexPrefill / XAttention /
    MInference papers report).  `mass`: (B, Hq, nbq, nbk) from block_attention_mass or a rank's rows-only share from
    ring_block_attention_mass; `mask`: a torch.bool mask that broadcasts against it (select_blocks' result, a ring rank's
    select_block_rows).  Plain torch, on the device of its arguments."""
    return (mass * mask.to(mass.dtype)).sum(dim=-1)


def hip_attn_forward(q, k, v, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1),
                     softcap=None, alibi_slopes=None, return_softmax=False, *, rng_state=None, sinks=None, cu_doclens=None,
                     bidirectional=None, block_mask=None, return_max_logits=False, block_select=None, return_block_mass=False):
    """`fwd-only` contract of the reference selector (kernels/__init__.py:63-65; call sites
    zigzag_ring_flash_attn.py:29-43, ring_flash_attn.py:36-48):
        (block_out (B,Sq,Hq,D) q.dtype, block_lse (B,Hq,Sq) fp32)
    Unlike the TORCH_* wrappers (attention.py:135) the LSE is NOT rounded to q.dtype.
    `dropout_p` > 0 needs `rng_state` = (seed, row0, key0, head0) or a bare seed (the contract returns no state; without it:
    NotImplementedError); the same state given to hip_attn_backward regenerates the mask.
    `sinks` (keyword only): one learned logit per query head, (Hq,) fp32 or q.dtype, in score units (not scaled): it joins every
    row's softmax denominator and carries no value; the returned lse includes it (include/usp_hip.h: usp_flash_fwd_sink).  Not
    together with softcap, alibi_slopes or dropout_p.
    `cu_doclens` (keyword only): the cumulative document lengths [0, e1, ..., Sq] of the sequence, host data (ring/doc_blocks.py):
    row i sees key j iff start(i) <= j <= i.  Needs causal=True and equally long q and k; not together with window_size, softcap,
    alibi_slopes, dropout_p or sinks.  None or the single document [0, Sq]: exactly the call without it.
    `bidirectional` (keyword only): half-open spans [(s, e), ...] of positions, host data, sorted and disjoint, each inside one
    document, or "documents" (ring/doc_blocks.py: parse_plan): inside a span every row sees the whole span, so row i sees key j
    iff start(i) <= j < hi(i).  With or without cu_doclens, under its preconditions and refusals.  None, an empty list or spans
    of length 1 only: exactly the call without it.
    `block_mask` (keyword only): a torch.bool DEVICE tensor (nb, nb), (Hq, nb, nb) or (B, Hq, nb, nb), nb = ceil(Sq / BLOCK_MASK_SIZE):
    row i sees key j iff block_mask[b, h, i // 128, j // 128] and (not causal or j <= i); under causal the bits above the diagonal
    are ignored.  It is never read on the host (it may come from a kernel on the same stream) and gets no gradient.  Needs
    equally long q and k; not together with any of window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens,
    bidirectional.  None: exactly the call without it.
    `return_max_logits` (keyword only): the result is (out, lse, max_logits), max_logits an fp32 (Hq,) device tensor without
    gradient: max over batch, rows i and the keys j row i sees of softmax_scale * q_i . k_j, in score units, -inf for a head whose
    rows see nothing (include/usp_hip.h: usp_flash_fwd_maxlogit; nothing is read on the host).  out and lse are those of the call
    without it on the two-waves-per-SIMD kernels.  Goes with window_size alone.  False: exactly the call without it.
    `block_select` (keyword only): a BlockSelect(top_k, keep_first=0, keep_local=1): exactly the call with
    block_mask=select_blocks(q, k, top_k, softmax_scale=, causal=, keep_first=, keep_local=) -- the same launches behind the two
    selection kernels, the same bits; or a BlockSelectTopP(top_p, keep_first=0, keep_local=1, share_group=False): likewise the
    call with block_mask=select_blocks_top_p(q, k, top_p, ...).  Not together with block_mask or anything block_mask refuses.  None: the call without it.
    (hip_attn_backward takes the mask, not the selection.)
    `return_block_mass` (keyword only): the result is (out, lse, mass), mass = block_attention_mass(q, k, lse, ...) of the call's
    own lse, computed behind the forward: fp32 (B, Hq, nb, nb) without gradient.  out and lse are bit for bit those of the call
    without it.  Goes with none of the other options and needs equally long q and k.  False: exactly the call without it."""
    if return_block_mass_alone(return_block_mass, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional,
                               block_mask, block_select, return_max_logits):
        block_mask_self_attention(q.shape[1], k.shape[1], "return_block_mass")
        out, lse = hip_attn_forward(q, k, v, softmax_scale=softmax_scale, causal=causal)
        return out, lse, block_attention_mass(q, k, lse, softmax_scale=softmax_scale, causal=causal)
    if max_logits_alone(return_max_logits, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional, block_mask,
                        block_select=block_select):
        B, Sq, Hq, D = q.shape
        scale = _default_scale(q, softmax_scale)
        if kernel_head_dim(D) != D:                 # zero padding changes no score
            out, lse, ml = hip_attn_forward(*pad_head_dim(q, k, v), softmax_scale=scale, causal=causal, window_size=window_size,
                                            return_max_logits=True)
            return out[..., :D].contiguous(), lse, ml
        out = torch.empty((B, Sq, Hq, D), dtype=q.dtype, device=q.device)
        lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=q.device)
        row_max = torch.empty((B, Hq, Sq), dtype=torch.float32, device=q.device)
        be = get_block_backend()
        be.fwd(q, k, v, scale, bool(causal), lse, out=out, window=window_of(window_size), row_max=row_max)
        return out, lse, be.row_max_reduce(row_max)
    if block_select_alone(block_select, block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional):
        block_mask = _selected(block_select, q, k, softmax_scale, causal)
    if block_mask_alone(block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional):
        block_mask_of(block_mask, q, k)
        B, Sq, Hq, D = q.shape
        scale = _default_scale(q, softmax_scale)
        if kernel_head_dim(D) != D:
            out, lse = hip_attn_forward(*pad_head_dim(q, k, v), softmax_scale=scale, causal=causal, block_mask=block_mask)
            return out[..., :D].contiguous(), lse
        out = torch.empty((B, Sq, Hq, D), dtype=q.dtype, device=q.device)
        lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=q.device)
        get_block_backend().fwd(q, k, v, scale, bool(causal), lse, out=out, bsp=block_mask)
        return out, lse
    f = Features.of(q, k, causal, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional=bidirectional)
    dr = _dropout_of(f.dropout, rng_state, "hip_attn_forward")
    B, Sq, Hq, D = q.shape
    scale = _default_scale(q, softmax_scale)
    if kernel_head_dim(D) != D:                 # e.g. 96: on zero-padded copies (kernel_head_dim)
        out, lse = hip_attn_forward(*pad_head_dim(q, k, v), dropout_p=dropout_p, softmax_scale=scale, causal=causal,
                                    window_size=window_size, softcap=f.softcap, alibi_slopes=alibi_slopes, rng_state=rng_state,
                                    sinks=sinks, cu_doclens=f.doc)
        return out[..., :D].contiguous(), lse
    out = torch.empty((B, Sq, Hq, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=q.device)
    be, kw = _block_call(f, q, dr)
    be.fwd(q, k, v, scale, bool(causal) and "span" not in kw, lse, out=out, **kw)
    return out, lse


def hip_attn_backward(dout, q, k, v, out, softmax_lse, block_dq_buffer, block_dk_buffer,
                      block_dv_buffer, dropout_p=0.0, softmax_scale=None, bwd_causal=False,
                      window_size=(-1, -1), softcap=None, alibi_slopes=None, deterministic=False,
                      rng_state=None, *args, sinks=None, dsinks=None, cu_doclens=None, bidirectional=None, block_mask=None,
                      **kwargs):
    """`bwd-only` contract (argument order of kernels/attention.py:205-206): writes dq/dk/dv into
    the caller's (possibly sliced, 16-bit) buffers; `out`/`softmax_lse` are the GLOBAL rows' values
    (zigzag_ring_flash_attn.py:115-137).  `dropout_p` > 0: `rng_state` as hip_attn_forward took it; `out` is the dropped one.
    `sinks` (keyword only) with `dsinks`, a contiguous fp32 (Hq,) buffer: `softmax_lse` is the sink-including one, dq / dk / dv
    come from the unchanged kernels, and dsinks[h] = -sum exp(sinks[h] - lse) * delta is written (usp_sink_bwd).
    `cu_doclens`, `bidirectional`, `block_mask` (keyword only): as hip_attn_forward took them."""
    bsp_kw = {}
    if block_mask_alone(block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional):
        bsp_kw = dict(bsp=block_mask_of(block_mask, q, k))
    f = Features.of(q, k, bwd_causal, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional=bidirectional)
    if sinks is not None and dsinks is None:
        raise ValueError("hip_attn_backward with sinks needs the fp32 (Hq,) buffer dsinks")
    dr = _dropout_of(f.dropout, rng_state, "hip_attn_backward")
    B, Sq, Hq, D = q.shape
    dev = q.device
    if kernel_head_dim(D) != D:                 # on zero-padded copies; the first D dims of the gradients are the answer
        pdo, pq, pk, pv, po = pad_head_dim(dout, q, k, v, out)
        g = [torch.empty_like(t) for t in (pq, pk, pv)]
        hip_attn_backward(pdo, pq, pk, pv, po, softmax_lse, g[0], g[1], g[2], dropout_p, _default_scale(q, softmax_scale),
                          bwd_causal, window_size, f.softcap, alibi_slopes, deterministic, rng_state, sinks=sinks, dsinks=dsinks,
                          cu_doclens=f.doc, block_mask=block_mask)
        for dst, src in zip((block_dq_buffer, block_dk_buffer, block_dv_buffer), g):
            dst.copy_(src[..., :D])
        return
    be, kw = _block_call(f, q, dr)
    delta = torch.empty((B, Hq, Sq), dtype=torch.float32, device=dev)
    be.delta(dout, out, delta)
    lse = softmax_lse if softmax_lse.dtype == torch.float32 else softmax_lse.float()
    if lse.stride(-1) != 1:
        lse = lse.contiguous()
    if sinks is not None:
        be.sink_grad(lse, delta, out=dsinks)
    # the kernels round the final result to 16 bits in their epilogues (no fp32 round trip + cast)
    def direct(t):
        return t.dim() == 4 and t.stride(3) == 1 and all(st % 4 == 0 for st in t.stride()[:3])
    tgt = [t if direct(t) else torch.empty(t.shape, dtype=t.dtype, device=dev)
           for t in (block_dq_buffer, block_dk_buffer, block_dv_buffer)]
    be.bwd(dout, q, k, v, lse, delta, None, None, None, _default_scale(q, softmax_scale), bool(bwd_causal) and "span" not in kw,
           dq16=tgt[0], dk16=tgt[1], dv16=tgt[2], **kw, **bsp_kw)
    for t, dst in zip(tgt, (block_dq_buffer, block_dk_buffer, block_dv_buffer)):
        if t is not dst:
            dst.copy_(t)


class _HipAttnFunc(torch.autograd.Function):
    """`fwd-bwd` stage: an autograd-aware single-device attention (what UlyssesAttention would use,
    yunchang/ulysses/attn_layer.py:48,101-113)."""

    @staticmethod
    def forward(ctx, q, k, v, softmax_scale, causal, return_lse, window_size=(-1, -1), softcap=None, alibi_slopes=None,
                dropout_p=0.0, dropout_head0=0, sinks=None, cu_doclens=None, block_mask=None, return_max_logits=False):
        scale = _default_scale(q, softmax_scale)
        q, k, v = kernel_operand(q), kernel_operand(k), kernel_operand(v)
        # dropout: one seed per call, drawn here, kept for the backward (draw_seed); the block is the whole sequence
        ctx.dropout_p = _C.dropout_value(dropout_p) or 0.0
        ctx.rng_state = (draw_seed(), 0, 0, int(dropout_head0)) if ctx.dropout_p else None
        out, lse, *ml = hip_attn_forward(q, k, v, dropout_p=ctx.dropout_p, softmax_scale=scale, causal=causal, window_size=window_size,
                                         softcap=softcap, alibi_slopes=alibi_slopes, rng_state=ctx.rng_state, sinks=sinks,
                                         cu_doclens=cu_doclens, block_mask=block_mask, return_max_logits=return_max_logits)
        ctx.cu_doclens = cu_doclens
        ctx.block_mask = block_mask                # (no gradient; the backward rebuilds its lists from it, on the device)
        ctx.has_sinks = sinks is not None          # (never beside slopes: the one optional saved tensor is either)
        ctx.save_for_backward(q, k, v, out, lse, *(() if alibi_slopes is None else (alibi_slopes,)),
                              *(() if sinks is None else (sinks,)))                                     # (slopes: no gradient,
        ctx.scale, ctx.causal, ctx.window_size, ctx.softcap = scale, bool(causal), window_size, softcap   # as in flash-attn)
        extra = ((lse,) if return_lse else ()) + tuple(ml)     # (ml: the max logits, a statistic the backward never sees)
        if extra:
            ctx.mark_non_differentiable(*extra)
            return (out,) + extra
        return out

    @staticmethod
    def backward(ctx, dout, *_):
        q, k, v, out, lse, *slopes = ctx.saved_tensors
        sinks = slopes.pop() if ctx.has_sinks else None
        dsinks = None if sinks is None else torch.empty(sinks.shape, dtype=torch.float32, device=q.device)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        hip_attn_backward(kernel_operand(dout), q, k, v, out, lse, dq, dk, dv, ctx.dropout_p, ctx.scale, ctx.causal,
                          ctx.window_size, ctx.softcap, slopes[0] if slopes else None, rng_state=ctx.rng_state, sinks=sinks,
                          dsinks=dsinks, cu_doclens=ctx.cu_doclens, block_mask=ctx.block_mask)
        if dsinks is not None:
            dsinks = dsinks.to(sinks.dtype) if ctx.needs_input_grad[11] else None
        return dq, dk, dv, None, None, None, None, None, None, None, None, dsinks, None, None, None


def hip_attn_func(q, k, v, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1),
                  softcap=0.0, alibi_slopes=None, deterministic=False, return_attn_probs=False,
                  *args, dropout_head0=0, sinks=None, cu_doclens=None, bidirectional=None, block_mask=None, return_max_logits=False,
                  block_select=None, return_block_mass=False, **kwargs):
    """`fwd-bwd` contract (flash_attn_func's signature): `out`, or `(out, softmax_lse, None)` with
    return_attn_probs (the probabilities themselves are never materialised, with dropout either: the third element stays
    None).  `softcap` > 0: flash-attn's tanh logit cap; None / 0 = off, a negative, NaN or infinite value raises ValueError.
    `alibi_slopes`: flash-attn's fp32 (Hq,) or (B, Hq) slopes (no gradient), not together with softcap.  `dropout_p` in (0, 1):
    the position-keyed mask of include/usp_hip.h under one seed per call from torch's default CPU generator (draw_seed), not
    together with softcap or alibi_slopes; NaN, a negative value or one >= 1 raises ValueError.  `dropout_head0` (keyword
    only): the global index of q's head 0 in the mask's counter (a Ulysses rank passes the first head it holds).
    `sinks` (keyword only): one learned logit per query head, (Hq,) fp32 or q.dtype (hip_attn_forward); it may require grad, and
    its gradient comes back in its own dtype and shape.  Not together with softcap, alibi_slopes or dropout_p.
    `cu_doclens` (keyword only): the document mask of a packed sequence (hip_attn_forward), padded head dims included.
    `bidirectional` (keyword only): bidirectional spans beside or without it (hip_attn_forward), likewise; parsed here once, the
    plan travels on as `cu_doclens`.
    `block_mask` (keyword only): a 128 x 128 block mask (hip_attn_forward), padded head dims included; no gradient.
    `return_max_logits` (keyword only): the result becomes `(out, max_logits)`, with return_attn_probs `(out, softmax_lse, None,
    max_logits)`: the fp32 (Hq,) per-head maximum of the visible pre-softmax logits (hip_attn_forward), padded head dims
    included; no gradient, never read on the host.  `out` and the gradients are those of the call without it.  Goes with
    window_size alone.
    `block_select` (keyword only): a BlockSelect or a BlockSelectTopP: the block mask is selected here, once, from the values
    of q and k (select_blocks / select_blocks_top_p; no gradient through the gate), and the call is the one with that block_mask: the autograd node keeps the mask
    for its backward, which never selects again.
    `return_block_mass` (keyword only): the result becomes `(out, mass)`, with return_attn_probs `(out, softmax_lse, None, mass)`:
    the fp32 (B, Hq, nb, nb) block-pooled attention map of the call (block_attention_mass on the call's own lse, computed under
    no_grad behind the forward), padded head dims included; no gradient, never read on the host.  `out`, the lse and the
    gradients are bit for bit those of the call without it.  Goes with none of the other options."""
    if return_block_mass_alone(return_block_mass, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional,
                               block_mask, block_select, return_max_logits):
        block_mask_self_attention(q.shape[1], k.shape[1], "return_block_mass")
        out, lse, _ = hip_attn_func(q, k, v, softmax_scale=softmax_scale, causal=causal, deterministic=deterministic,
                                    return_attn_probs=True)
        mass = block_attention_mass(q, k, lse, softmax_scale=softmax_scale, causal=causal)
        return (out, lse, None, mass) if return_attn_probs else (out, mass)
    if max_logits_alone(return_max_logits, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional, block_mask,
                        block_select=block_select):
        D = q.shape[-1]
        scale = _default_scale(q, softmax_scale)                 # (of the unpadded head dim)
        res = _HipAttnFunc.apply(*pad_head_dim(q, k, v), scale, causal, bool(return_attn_probs), window_size, None, None, 0.0, 0,
                                 None, None, None, True)
        out = res[0] if kernel_head_dim(D) == D else res[0][..., :D]
        return (out, res[1], None, res[2]) if return_attn_probs else (out, res[1])
    if block_select_alone(block_select, block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional):
        block_mask = _selected(block_select, q, k, softmax_scale, causal)
    if block_mask_alone(block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional):
        block_mask_of(block_mask, q, k)
        D = q.shape[-1]
        if kernel_head_dim(D) != D:
            res = hip_attn_func(*pad_head_dim(q, k, v), softmax_scale=_default_scale(q, softmax_scale), causal=causal,
                                return_attn_probs=return_attn_probs, block_mask=block_mask)
            return (res[0][..., :D], res[1], None) if return_attn_probs else res[..., :D]
        res = _HipAttnFunc.apply(q, k, v, softmax_scale, causal, bool(return_attn_probs), (-1, -1), None, None, 0.0, 0, None, None,
                                 block_mask)
        return (res[0], res[1], None) if return_attn_probs else res
    f = Features.of(q, k, causal, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional=bidirectional)
    cap, cu_doclens = f.softcap, f.doc
    D = q.shape[-1]
    if kernel_head_dim(D) != D:                 # on zero-padded copies (autograd differentiates the pad and the slice)
        res = hip_attn_func(*pad_head_dim(q, k, v), dropout_p=dropout_p, softmax_scale=_default_scale(q, softmax_scale),
                            causal=causal, window_size=window_size, softcap=cap, alibi_slopes=alibi_slopes,
                            return_attn_probs=return_attn_probs, dropout_head0=dropout_head0, sinks=sinks, cu_doclens=cu_doclens)
        return (res[0][..., :D], res[1], None) if return_attn_probs else res[..., :D]
    if return_attn_probs:
        out, lse = _HipAttnFunc.apply(q, k, v, softmax_scale, causal, True, window_size, cap, alibi_slopes, dropout_p, dropout_head0,
                                      sinks, cu_doclens)
        return out, lse, None
    return _HipAttnFunc.apply(q, k, v, softmax_scale, causal, False, window_size, cap, alibi_slopes, dropout_p, dropout_head0,
                              sinks, cu_doclens)
