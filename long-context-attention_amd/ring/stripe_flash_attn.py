"""Stripe ring attention: same surface as yunchang/ring/stripe_flash_attn.py.

Layout: token t lives on ring rank t % P (EXTRACT_FUNC_DICT["strip"]), so every ring step is a
causal block and the work is balanced without the zigzag pairing.  With local index i <-> global
token i*P + r, the K/V of ring rank r_k = r - step are visible to query i iff
    i_k <= i       when r_k <= r   (step <= rank:  plain causal square,        stripe:31-47)
    i_k <= i - 1   when r_k >  r   (step >  rank:  q[:, 1:] x k[:, :-1] causal, :48-66; rows 1: only)
Both shapes are what the HIP kernel already does (bottom-right aligned causal on a square block);
the row offset is a pointer offset on q / out / acc / lse.  Differences from the reference are the
ones listed in zigzag_ring_flash_attn.py (fused merge, fp32 in-place gradients, side-stream relay).

A block mask (`block_mask`, ring/front_end.py: BlockMask, riding in the `cu_doclens` slot) is served at ring degree 1 only, and there
by the BASIC ring's forward / backward (ring_front_end: ring_pair) -- one block over the natural order; beyond degree 1 the front
end refuses and names the basic ring.
"""
import torch
import torch.distributed as dist

from ..kernels import AttnType
from ..kernels.attention import RowMaxBackend, get_block_backend
from .front_end import DENSE_RING, ring_dropout, ring_front_end
from .utils import FULL, KVRelay, group_info, final_grads, travel_dkdv


def stripe_fwd_step(be, r, P, step, q, kk, vv, softmax_scale, lse, out, acc):
    """One ring step of the forward (pure schedule logic; also driven by single-GPU tests)."""
    S = q.shape[1]
    last = step == P - 1
    if step <= r:
        # row 0 gets its last update at step r, rows 1: at step P-1
        fe = S if last else (1 if step == r else 0)
        be.fwd(q, kk, vv, softmax_scale, True, lse, out, acc, step > 0, 0, fe)
    elif S > 1:
        be.fwd(q[:, 1:], kk[:, :-1], vv[:, :-1], softmax_scale, True, lse[:, :, 1:], out[:, 1:],
               acc[:, 1:], True, 0, S - 1 if last else 0)


def stripe_bwd_block(be, r, P, step, dout, q, kk, vv, lse, delta, softmax_scale, dq_acc, dk_dst, dv_dst):
    if step <= r:                                  # stripe_flash_attn.py:116-136
        be.bwd(dout, q, kk, vv, lse, delta, dq_acc, dk_dst, dv_dst, softmax_scale, True,
               accum_dq=step > 0)
    elif q.shape[1] > 1:                           # :137-160
        be.bwd(dout[:, 1:], q[:, 1:], kk[:, :-1], vv[:, :-1], lse[:, :, 1:], delta[:, :, 1:],
               dq_acc[:, 1:], dk_dst[:, :-1], dv_dst[:, :-1], softmax_scale, True, accum_dq=True)


def stripe_bwd_fold(be, r, step, dk_acc, dv_acc, dk_blk, dv_blk):
    if step <= r:                                  # :176-178
        be.add(dk_acc, dk_acc, dk_blk)
        be.add(dv_acc, dv_acc, dv_blk)
    elif dk_acc.shape[1] > 1:                      # :179-181
        be.add(dk_acc[:, :-1], dk_acc[:, :-1], dk_blk[:, :-1])
        be.add(dv_acc[:, :-1], dv_acc[:, :-1], dv_blk[:, :-1])


def stripe_flash_attn_forward(process_group, q, k, v, softmax_scale, dropout_p=0, causal=True,
                              window_size=(-1, -1), softcap=0.0, alibi_slopes=None, deterministic=False,
                              attn_type: AttnType = AttnType.HIP, overlap=False, rng_state=None, sinks=None, max_logits=False):
    assert causal, "stripe flash attn only supports causal attention, if not causal, use ring flash attn instead"
    P, r = group_info(dist, process_group)
    assert alibi_slopes is None or P == 1, "ALiBi: this ring places one block only (ring/front_end.py: _place)"
    dr = ring_dropout(dropout_p, rng_state)      # (p, seed, head0) | None: ring degree 1 only (ring/front_end.py: _place)
    assert dr is None or P == 1, "dropout: this ring places one block only (ring/front_end.py: _place)"
    # `sinks`: one logit per query head, on the launch that opens the rows' state (step 0, every row), at any ring degree
    be = get_block_backend(beside_transfers=P > 1 or overlap, softcap=softcap, alibi=alibi_slopes, dropout=dr, sinks=sinks)
    # `max_logits` (ring/front_end.py: return_max_logits): (out, lse, max_logits) -- every launch, the `rows 1:` ones included, leaves
    # the row maxima where its lse goes (kernels/attention.py: RowMaxBackend); one reduce at the end: this rank's rows, fp32 (Hq,)
    if max_logits:
        assert alibi_slopes is None and dr is None and sinks is None, "return_max_logits: kernels/features.py: max_logits_alone"
        be = RowMaxBackend(be)
    B, S, H, D = q.shape
    dev = q.device
    out = torch.empty((B, S, H, D), dtype=q.dtype, device=dev)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    acc = torch.empty((B, S, H, D), dtype=torch.float32, device=dev) if P > 1 else None
    with KVRelay(process_group, k, v) as relay:
        for step in range(P):
            kk, vv = relay.get(step)
            stripe_fwd_step(be, r, P, step, q, kk, vv, softmax_scale, lse, out, acc)
    return (out, lse, be.max_logits(lse)) if max_logits else (out, lse)


def stripe_flash_attn_backward(process_group, dout, q, k, v, out, softmax_lse, softmax_scale,
                               dropout_p=0, causal=True, window_size=(-1, -1), softcap=0.0,
                               alibi_slopes=None, deterministic=False, attn_type: AttnType = AttnType.HIP,
                               overlap=False, defer=None, rng_state=None, sinks=None):
    assert causal, "stripe flash attn only supports causal attention, if not causal, ring flash attn instead"
    P, r = group_info(dist, process_group)
    assert alibi_slopes is None or P == 1, "ALiBi: this ring places one block only (ring/front_end.py: _place)"
    dr = ring_dropout(dropout_p, rng_state)
    assert dr is None or P == 1, "dropout: this ring places one block only (ring/front_end.py: _place)"
    be = get_block_backend(beside_transfers=P > 1 or overlap, softcap=softcap, alibi=alibi_slopes, dropout=dr, sinks=sinks)
    B, S, H, D = q.shape
    dev = q.device
    delta = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    be.delta(dout, out, delta)
    # sinks: this rank's share of their gradient (its rows) from the global lse, a fourth fp32 element of the result
    with_dsinks = (lambda g: g) if sinks is None else (lambda g, ds=be.sink_grad(softmax_lse, delta): tuple(g) + (ds,))
    if P == 1:
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        be.bwd(dout, q, k, v, softmax_lse, delta, None, None, None, softmax_scale, True,
               dq16=dq, dk16=dk, dv16=dv)
        return with_dsinks((dq, dk, dv))
    dq_acc = torch.empty((B, S, H, D), dtype=torch.float32, device=dev)

    def block(step, kk, vv, dk_dst, dv_dst):
        stripe_bwd_block(be, r, P, step, dout, q, kk, vv, softmax_lse, delta, softmax_scale, dq_acc,
                         dk_dst, dv_dst)

    def fold(step, dk_acc, dv_acc, dk_blk, dv_blk):
        stripe_bwd_fold(be, r, step, dk_acc, dv_acc, dk_blk, dv_blk)

    # steps > rank see k[:, :-1] only (:137-160, :179-181); a one-token shard has nothing to do there
    dk_acc, dv_acc = travel_dkdv(process_group, k, v, block, fold, be=be, final_dtype=k.dtype, defer=defer,
                                 extent=lambda rank, step: FULL if step <= rank else (slice(0, S - 1) if S > 1 else None))
    return with_dsinks(final_grads(be, (q, k, v), (dq_acc, dk_acc, dv_acc)))


(StripeFlashAttnFunc, stripe_flash_attn_func, stripe_flash_attn_kvpacked_func, stripe_flash_attn_qkvpacked_func) = ring_front_end(
    "stripe_flash_attn", "StripeFlashAttnFunc", stripe_flash_attn_forward, stripe_flash_attn_backward, DENSE_RING)
