"""Basic (contiguous-layout) ring attention: same surface as yunchang/ring/ring_flash_attn.py.

Block structure as the reference (:29-56 forward, :93-143 backward): ring step s sees the K/V of
ring rank r-s; under causal only steps <= r compute and only step 0 is causal.  At ring degree 1
(BASELINE configs C2, C3) this is one kernel call.  The MI355X-first differences are those listed
in zigzag_ring_flash_attn.py (fused merge, fp32 in-place gradient accumulation, K/V relay on a
side stream); additionally dq is returned in q.dtype (the reference hard-codes bfloat16 at :147).

ALiBi (`alibi_slopes`) is one block at ring degree 1; at ring degree > 1 it is served on request (USP_RING_ALIBI=global) over
GLOBAL positions: the step that sees the K/V of ring rank kr is launched with the diagonal shift (r - kr) * S, which places the
bias of the block (include/usp_hip.h: usp_flash_fwd_alibi) -- K/V transport and the dK/dV return are unchanged.

Dropout (`dropout_p`) is served at any ring degree, by default: the mask is a function of GLOBAL positions (include/usp_hip.h:
usp_flash_fwd_dropout), so the step that sees the K/V of ring rank kr is launched with `at=(r * S, kr * S)` -- where its rows and
keys lie in the whole sequence -- forward and backward alike, and the ring's result is the single-device one for the same seed.
(The reference forwards dropout_p to every block and drops the rng state in its backward, :112-119.)

A sliding window (`window_size`) is one windowed block at ring degree 1; at ring degree > 1 it is served on request
(USP_RING_WINDOW=global) over GLOBAL positions: only the blocks the window touches are fetched, launched and returned, each
with its own shifted bounds (ring/window_blocks.py).

A document mask (`cu_doclens`, ring/doc_blocks.py) is served at any ring degree, by default: rank r holds the global rows
[r S, (r + 1) S), and the step that sees the K/V of ring rank kr is launched with the (row_lo, key_hi) arrays of (those rows, the
keys [kr S, (kr + 1) S)) -- the diagonal block causal, the blocks below it full with a left bound.  A block in which nothing is
visible (start(r S) >= (kr + 1) S) is not launched: the rows' running state is untouched and its dK/dV block is zero.  The
diagonal block always sees something and stays first, so it opens the rows' state; the transfers stay as they are.

Bidirectional spans (`bidirectional`, riding inside the parsed `cu_doclens` plan: ring/doc_blocks.py) are served at any ring
degree too: every launch takes the four arrays of (its rows, its keys) as `span=` and runs non-causal -- the diagonal lies in
row_hi.  Where no span straddles a shard boundary the live blocks are the document ring's and its schedule is kept as it is.
A span across a boundary makes a block ABOVE the diagonal live (kr > r; a span longer than a shard several): such a call takes
the planned direct transport of the windowed ring -- one grouped send / recv of K/V with the peers of the plan
(doc_blocks.SpanRingPlan: which (rank, step) blocks are live is host arithmetic any rank does for any other), every dK/dV block
straight to its owner, added there in step order, so two identical calls give the same bits.
"""
import os

import torch
import torch.distributed as dist

from ..kernels import AttnType
from ..kernels.attention import RowMaxBackend, get_block_backend, window_of
from . import block_pieces, doc_blocks
from .front_end import BASIC_RING, BlockMask, ring_dropout, ring_front_end
from .utils import FULL, KVRelay, group_info, final_grads, return_dkdv_direct, travel_dkdv
from .window_blocks import WindowPlan


def ring_window_mode() -> str:
    """USP_RING_WINDOW, read per call: "global" serves a sliding window at ring degree > 1 with GLOBAL semantics (row i of
    the whole sequence sees key j iff i - left <= j <= i + right); anything else (the default) refuses."""
    return os.environ.get("USP_RING_WINDOW", "").strip().lower()


def _ring_window(window_size, P):
    """flash-attn's window_size -> (left, right) | None.  A window is served where the ring has ONE block (ring degree
    1: the Ulysses-only layouts, the single-GPU path).  Across ring steps every block needs its own shifted bounds
    (ring/window_blocks.py; the reference hands the same `window_size` to every block, kernels/attention.py:165-202 --
    correct at ring degree 1 only, a different function beyond).  That is served on request, USP_RING_WINDOW=global: a
    caller who comes from the reference gets an error, not other numbers, until they ask."""
    win = window_of(window_size)
    if win is not None and P > 1 and ring_window_mode() != "global":
        raise NotImplementedError("sliding-window attention across ring steps (ring degree > 1) is not supported by default: "
                                  "set USP_RING_WINDOW=global for a window over GLOBAL positions on the basic ring (the "
                                  "reference applies the same window to every block instead, a different function)")
    return win


def ring_alibi_mode() -> str:
    """USP_RING_ALIBI, read per call: "global" serves alibi_slopes at ring degree > 1 with distances between GLOBAL positions
    (row i and key j of the whole sequence: -slope * |i - j|); anything else (the default) refuses."""
    return os.environ.get("USP_RING_ALIBI", "").strip().lower()


def _ring_alibi(alibi_slopes, P):
    """flash-attn's alibi_slopes as the block launches take them, or None.  One block (ring degree 1) is flash-attn's own
    function.  Across ring steps every block needs its own diagonal (the reference hands the same slopes to every block,
    yunchang/ring/ring_flash_attn.py:36-48, and so measures distances INSIDE each block: a different function).  Global
    positions are served on request, USP_RING_ALIBI=global: a caller who comes from the reference gets an error, not other
    numbers, until they ask."""
    if alibi_slopes is not None and P > 1 and ring_alibi_mode() != "global":
        raise NotImplementedError("alibi_slopes across ring steps (ring degree > 1) is not supported by default: set "
                                  "USP_RING_ALIBI=global for a bias over GLOBAL positions on the basic ring (the reference "
                                  "applies the same per-block bias to every block instead, a different function)")
    return alibi_slopes


def _step_launch_kw(al, dr, r, P, step, S, blk_kw=None):
    """The keywords that place the launch of ring step `step` in the whole sequence.  The block holds the K/V of ring rank
    kr = r - step (mod P); this rank's queries start at global row r * S, the block's keys at global key kr * S.
      - dropout (`dr` not None): `at=(r * S, kr * S)`, the global position of the block's row 0 and key 0 -- the mask is a function
        of global positions (include/usp_hip.h: usp_flash_fwd_dropout), forward and backward alike;
      - ALiBi (`al` not None): `shift=(r - kr) * S`, by which the block's keys lie in front of this rank's queries (behind them:
        negative, the non-causal ring).  The rank's own block (shift 0) carries no keyword: it is an unshifted launch and keeps
        its automatic K split and cuts.
    `blk_kw`: the launch keywords of a window planner's block; a bounded block carries its own shift, which places the MASK --
    the same number by construction (ring/window_blocks.py: (rank - src) * c), asserted because the bias would follow it."""
    blk_kw = dict(blk_kw or {})
    if dr is not None:
        blk_kw["at"] = (r * S, ((r - step) % P) * S)
    if al is None:
        return blk_kw
    shift = (r - (r - step) % P) * S
    assert blk_kw.get("shift", shift) == shift, f"ring step {step}: the window block's shift {blk_kw['shift']} is not the bias's {shift}"
    if shift != 0:
        blk_kw["shift"] = shift
    return blk_kw


def _block_mask_of(cu_doclens):
    """(the BlockMask that rides in the cu_doclens slot | None, the document plan | None)"""
    return (cu_doclens, None) if isinstance(cu_doclens, BlockMask) else (None, cu_doclens)


def _bsp_kw(bm, r, P, step, S):
    """The `bsp=` keyword of the launch of ring step `step` under a block mask: the view of the global mask that holds this
    rank's row blocks against the key blocks of ring rank kr = r - step (mod P) -- a strided view, no copy, never read here.
    The schedule is untouched: the diagonal block is causal, the blocks below it full, and a block whose sub-mask is all false
    is launched all the same (skipping it would need a host read of the mask); the kernels return quickly on empty lists."""
    return {} if bm is None else {"bsp": bm.view(r, (r - step) % P, S, P)}


def _window_plan(win, P, r, c, causal):
    return WindowPlan(P, c, bool(causal), win[0], win[1], r)


def _window_kw(win):
    return {} if win is None else {"window": win}


def basic_fwd_step(be, r, P, step, causal, q, kk, vv, softmax_scale, lse, out, acc, **kw):
    """One step of the contiguous-layout ring forward (ring_flash_attn.py:29-56); pure schedule
    logic, also driven by the single-GPU tests with virtual ranks.  `kw`: further keywords of the launch (ALiBi: shift)."""
    if causal and step > r:
        return
    last_compute = r if causal else P - 1
    fe = q.shape[1] if step == last_compute else 0
    be.fwd(q, kk, vv, softmax_scale, bool(causal and step == 0), lse, out, acc, step > 0, 0, fe, **kw)


def basic_bwd_block(be, r, P, step, causal, dout, q, kk, vv, lse, delta, softmax_scale, dq_acc,
                    dk_dst, dv_dst, **kw):
    """Block backward of one step (:93-122).  Returns False when the step computes nothing.  `kw`: as basic_fwd_step."""
    if causal and step > r:
        return False
    be.bwd(dout, q, kk, vv, lse, delta, dq_acc, dk_dst, dv_dst, softmax_scale,
           bool(causal and step == 0), accum_dq=step > 0, **kw)
    return True


def ring_flash_attn_forward(process_group, q, k, v, softmax_scale, dropout_p=0, causal=True,
                            window_size=(-1, -1), softcap=0.0, alibi_slopes=None, deterministic=False,
                            attn_type: AttnType = AttnType.HIP, attn_processor=None, overlap=False, first=None, tail=None,
                            rng_state=None, sinks=None, cu_doclens=None, max_logits=False):
    """`cu_doclens`: the parsed document lists of the whole sequence (ring/front_end.py: _place), None = off.
    `max_logits` (ring/front_end.py: return_max_logits; beside a window alone): the result is (out, lse, max_logits) -- every launch
    leaves the row maxima where its lse goes (kernels/attention.py: RowMaxBackend) and ONE reduce at the end gives this rank's
    share, fp32 (Hq,): the maximum over its rows.
    `rng_state` = (seed, head0) with dropout_p > 0 (ring/front_end.py draws it).  `sinks`: one logit per query head; it rides on
    the launch that opens the rows' state (step 0; the window planner's first block), at any ring degree.  `overlap`, `first`, `tail`: the caller has exchanges of its own in flight (the head-group pipeline), see
    zigzag_ring_flash_attn_forward.  This ring serves `first` and `tail` at ring degree 1 only (ring/block_pieces.py)."""
    P, r = group_info(dist, process_group)
    bm, cu_doclens = _block_mask_of(cu_doclens)
    pieces = first is not None or tail is not None
    assert bm is None or not pieces, "block_mask: ring/front_end.py"
    dr = ring_dropout(dropout_p, rng_state)
    assert not pieces or (P == 1 and causal and window_of(window_size) is None and alibi_slopes is None and dr is None)
    al = _ring_alibi(alibi_slopes, P)
    block_pieces.refuse_sinks(sinks, pieces)
    assert cu_doclens is None or (causal and not pieces and window_of(window_size) is None), "cu_doclens: ring/front_end.py: _place"
    be = get_block_backend(beside_transfers=P > 1 or overlap or pieces, softcap=softcap, alibi=al, dropout=dr, sinks=sinks,
                           doc=cu_doclens)
    if max_logits:
        assert not pieces and bm is None and cu_doclens is None and al is None and dr is None and sinks is None, \
            "return_max_logits: kernels/features.py: max_logits_alone"
        be = RowMaxBackend(be)
    if pieces:
        return block_pieces.forward_in_pieces(be, q, k, v, softmax_scale, first, tail)
    B, S, H, D = q.shape
    dev = q.device
    out = torch.empty((B, S, H, D), dtype=q.dtype, device=dev)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    done = (lambda: (out, lse, be.max_logits(lse))) if max_logits else (lambda: (out, lse))
    if cu_doclens is not None:       # the document mask: the steps with something visible, each with its own arrays
        assert k.shape[1] == S, "the basic ring holds equally long chunks of q and k"
        call = doc_blocks.ring_call(cu_doclens, S, P, r, dev)
        if P > 1 and doc_blocks.spans_cross_shards(cu_doclens, S, P):   # a live block above the diagonal: the planned transport
            plan = doc_blocks.SpanRingPlan(cu_doclens, S, P, r)
            acc = torch.empty((B, S, H, D), dtype=torch.float32, device=dev) if len(plan.steps) > 1 else None
            with KVRelay(process_group, k, v, recv_steps=plan.recv, send_steps=plan.send) as relay:
                for i, step in enumerate(plan.steps):                  # (step 0, the diagonal block, is always the first)
                    kk, vv = relay.get(step)
                    be.fwd(q, kk, vv, softmax_scale, False, lse, out, acc, i > 0, 0, S if step == plan.steps[-1] else 0,
                           **call.kw(step))
            return out, lse
        steps = [s for s in range(r + 1) if call.visible(s)]          # (step 0, the diagonal block, is always among them)
        acc = torch.empty((B, S, H, D), dtype=torch.float32, device=dev) if len(steps) > 1 else None
        with KVRelay(process_group, k, v) as relay:
            for step in range(P):
                kk, vv = relay.get(step)
                if step in steps:
                    be.fwd(q, kk, vv, softmax_scale, call.causal(step, step == 0), lse, out, acc, step > 0, 0,
                           S if step == steps[-1] else 0, **call.kw(step))
        return out, lse
    win = _ring_window(window_size, P)
    if win is not None and P == 1:   # ring degree 1: one block, the kernels take flash-attn's window (left, right)
        be.fwd(q, k, v, softmax_scale, bool(causal), lse, out, window=win)
        return done()
    assert bm is None or (win is None and k.shape[1] == S), "block_mask: ring/front_end.py"
    if win is not None:              # USP_RING_WINDOW=global: only the blocks the window touches, each with its own bounds
        assert k.shape[1] == S, "the basic ring holds equally long chunks of q and k"
        plan = _window_plan(win, P, r, S, causal)
        acc = torch.empty((B, S, H, D), dtype=torch.float32, device=dev) if len(plan.steps) > 1 else None
        with KVRelay(process_group, k, v, recv_steps=plan.recv, send_steps=plan.send) as relay:
            for i, step in enumerate(plan.steps):
                kk, vv = relay.get(step)
                blk = plan.block(step)
                be.fwd(q, kk, vv, softmax_scale, blk.causal, lse, out, acc, i > 0, 0, S if step == plan.steps[-1] else 0,
                       **_step_launch_kw(al, dr, r, P, step, S, blk.launch_kw()))
        return done()
    last_compute = r if causal else P - 1
    acc = torch.empty((B, S, H, D), dtype=torch.float32, device=dev) if last_compute > 0 else None
    with KVRelay(process_group, k, v) as relay:
        for step in range(P):
            kk, vv = relay.get(step)
            basic_fwd_step(be, r, P, step, causal, q, kk, vv, softmax_scale, lse, out, acc,
                           **_step_launch_kw(al, dr, r, P, step, S), **_bsp_kw(bm, r, P, step, S))
    return done()


def ring_flash_attn_backward(process_group, dout, q, k, v, out, softmax_lse, softmax_scale,
                             dropout_p=0, causal=True, window_size=(-1, -1), softcap=0.0,
                             alibi_slopes=None, deterministic=False,
                             attn_type: AttnType = AttnType.HIP, overlap=False, defer=None, first=None, dq_first=None,
                             rng_state=None, sinks=None, cu_doclens=None):
    """`cu_doclens`: as the forward's.  `rng_state`: as the forward's (the same state regenerates its mask).  `sinks`: as the forward's; `softmax_lse` holds them, the
    block kernels are unchanged, and this rank's share of their gradient (its rows) is returned as a fourth, fp32 element.  `defer`: travel_dkdv's list for the pending last hop.  `first`, `dq_first`: see zigzag_ring_flash_attn_backward; served at
    ring degree 1 only (ring/block_pieces.py)."""
    P, r = group_info(dist, process_group)
    bm, cu_doclens = _block_mask_of(cu_doclens)
    pieces = first is not None or dq_first is not None
    assert bm is None or (not pieces and window_of(window_size) is None), "block_mask: ring/front_end.py"
    dr = ring_dropout(dropout_p, rng_state)
    assert not pieces or (P == 1 and causal and window_of(window_size) is None and alibi_slopes is None and dr is None)
    al = _ring_alibi(alibi_slopes, P)
    block_pieces.refuse_sinks(sinks, pieces)
    assert cu_doclens is None or (causal and not pieces and window_of(window_size) is None), "cu_doclens: ring/front_end.py: _place"
    be = get_block_backend(beside_transfers=P > 1 or overlap or pieces, softcap=softcap, alibi=al, dropout=dr, sinks=sinks,
                           doc=cu_doclens)
    if pieces:
        return block_pieces.backward_in_pieces(be, dout, q, k, v, out, softmax_lse, softmax_scale, first, dq_first)
    B, S, H, D = q.shape
    dev = q.device
    delta = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    be.delta(dout, out, delta)
    with_dsinks = (lambda g: g) if sinks is None else (lambda g, ds=be.sink_grad(softmax_lse, delta): tuple(g) + (ds,))
    call = None if cu_doclens is None else doc_blocks.ring_call(cu_doclens, S, P, r, dev)
    if P == 1:   # one block: the kernels round the gradients to q.dtype in their epilogues
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        be.bwd(dout, q, k, v, softmax_lse, delta, None, None, None, softmax_scale,
               bool(causal) if call is None else call.causal(0, causal),
               dq16=dq, dk16=dk, dv16=dv, **_window_kw(_ring_window(window_size, P)), **({} if call is None else call.kw(0)),
               **_bsp_kw(bm, 0, 1, 0, q.shape[1]))
        return with_dsinks((dq, dk, dv))
    win = _ring_window(window_size, P)
    dq_acc = torch.empty((B, S, H, D), dtype=torch.float32, device=dev)
    if win is not None:              # USP_RING_WINDOW=global: every block straight to its owner, only the rows it has gradients for
        # (`defer` is not used here: it hands the travelling accumulators' last hop to the head-group pipeline, which takes no
        # window; every transfer of this path is waited for on this stream before it returns)
        plan = _window_plan(win, P, r, S, causal)

        def win_block(step, kk, vv, dk_dst, dv_dst):
            blk = plan.block(step)
            be.bwd(dout, q, kk, vv, softmax_lse, delta, dq_acc, dk_dst, dv_dst, softmax_scale, blk.causal,
                   accum_dq=step > 0, **_step_launch_kw(al, dr, r, P, step, S, blk.launch_kw()))   # (step 0 is never empty: it is the first to write dq)

        dk_acc, dv_acc = return_dkdv_direct(process_group, k, v, win_block, plan.key_extent, be,
                                            relay_kw=dict(recv_steps=plan.recv, send_steps=plan.send))
        return with_dsinks(final_grads(be, (q, k, v), (dq_acc, dk_acc, dv_acc)))

    if call is not None and doc_blocks.spans_cross_shards(cu_doclens, S, P):
        # spans across a shard boundary: blocks above the diagonal are live -- every live block straight to its owner
        plan = doc_blocks.SpanRingPlan(cu_doclens, S, P, r)

        def span_block(step, kk, vv, dk_dst, dv_dst):
            be.bwd(dout, q, kk, vv, softmax_lse, delta, dq_acc, dk_dst, dv_dst, softmax_scale, False,
                   accum_dq=step > 0, **call.kw(step))                 # (step 0 is never empty: it is the first to write dq)

        dk_acc, dv_acc = return_dkdv_direct(process_group, k, v, span_block, plan.key_extent, be,
                                            relay_kw=dict(recv_steps=plan.recv, send_steps=plan.send))
        return with_dsinks(final_grads(be, (q, k, v), (dq_acc, dk_acc, dv_acc)))

    def block(step, kk, vv, dk_dst, dv_dst):
        if call is not None:          # the document mask: a step in which nothing is visible computes nothing
            if step > r or not call.visible(step):
                return False
            if doc_blocks.spans_of(cu_doclens) is not None:           # (the diagonal lies in row_hi: never causal)
                be.bwd(dout, q, kk, vv, softmax_lse, delta, dq_acc, dk_dst, dv_dst, softmax_scale, False,
                       accum_dq=step > 0, **call.kw(step))
                return True
            return basic_bwd_block(be, r, P, step, causal, dout, q, kk, vv, softmax_lse, delta, softmax_scale,
                                   dq_acc, dk_dst, dv_dst, doc=call.doc(step))
        return basic_bwd_block(be, r, P, step, causal, dout, q, kk, vv, softmax_lse, delta, softmax_scale,
                               dq_acc, dk_dst, dv_dst, **_step_launch_kw(al, dr, r, P, step, S), **_bsp_kw(bm, r, P, step, S))

    def fold(step, dk_acc, dv_acc, dk_blk, dv_blk):
        be.add(dk_acc, dk_acc, dk_blk)
        be.add(dv_acc, dv_acc, dv_blk)

    # under causal only steps <= rank compute (:93-122)
    dk_acc, dv_acc = travel_dkdv(process_group, k, v, block, fold, be=be, final_dtype=k.dtype, defer=defer,
                                 extent=lambda rank, step: None if (causal and step > rank) or
                                 (cu_doclens is not None and not doc_blocks.ring_visible(cu_doclens, S, rank, step, P)) else FULL)
    return with_dsinks(final_grads(be, (q, k, v), (dq_acc, dk_acc, dv_acc)))


(RingFlashAttnFunc, ring_flash_attn_func, ring_flash_attn_kvpacked_func, ring_flash_attn_qkvpacked_func) = ring_front_end(
    "ring_flash_attn", "RingFlashAttnFunc", ring_flash_attn_forward, ring_flash_attn_backward, BASIC_RING,
    attn_processor=True)
