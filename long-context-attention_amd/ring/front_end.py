"""The public front end of every ring: ONE autograd Function and ONE *_func / *_kvpacked_func / *_qkvpacked_func trio,
made per ring from its (forward, backward) pair.  The ring modules keep their schedules and bind their public names to what
`ring_front_end` returns; the surfaces are the reference's (yunchang/ring/*.py), argument for argument."""
import torch
import torch.distributed as dist

from .._C import alibi_value, dropout_value, sinks_value, softcap_value
from ..kernels import AttnType
from ..kernels.attention import draw_seed, kernel_head_dim, kernel_operand, needs_grad, pad_head_dim
from . import doc_blocks
from .utils import group_info
from .varlen_utils import unflatten_lse


def _check_hot_path_args(dropout_p, window_size, softcap):
    """Refuses what the ring schedules do not serve.  softcap IS served (a per-score transform: every block launch carries
    it, get_block_backend); a negative, NaN or infinite one raises ValueError (flash-attn ignores a negative one)."""
    if dropout_p not in (0, 0.0):
        raise NotImplementedError("dropout_p != 0 is not supported by the HIP ring attention")
    if window_size is not None and tuple(window_size) != (-1, -1):
        raise NotImplementedError("sliding-window attention is not supported by this HIP ring attention (zigzag, stripe and "
                                  "varlen rings, the async layer): use the basic ring (ring_impl_type=\"basic\", "
                                  "ring_flash_attn_func), which serves a window at ring degree 1 and, with "
                                  "USP_RING_WINDOW=global, across ring steps")
    softcap_value(softcap)


def _check_alibi(alibi_slopes, q, softcap, group, packed, served_beyond_one_block):
    """ALiBi (flash-attn's alibi_slopes) on a ring.  The bias of a block depends on where the block lies in the whole sequence,
    so a ring serves it only where it places every block: the dense rings at ring degree 1 (ONE block: basic, zigzag, stripe)
    and the basic ring beyond (`served_beyond_one_block`: its forward decides, USP_RING_ALIBI=global).  Everything else refuses;
    a wrong shape, dtype or device of the slopes is a ValueError (_C.alibi_value)."""
    if alibi_slopes is None:
        return
    if packed:
        raise NotImplementedError("alibi_slopes is not supported by the variable-length (packed) rings: use the basic ring "
                                  "(ring_impl_type=\"basic\", ring_flash_attn_func) on dense batches")
    if softcap_value(softcap) is not None:
        raise NotImplementedError("alibi_slopes together with softcap is not supported by the HIP attention kernels")
    alibi_value(alibi_slopes, q.shape[0], q.shape[2], q.device)
    if not served_beyond_one_block and group_info(dist, group)[0] > 1:
        raise NotImplementedError("alibi_slopes across ring steps (ring degree > 1) is not supported by the zigzag and stripe "
                                  "rings: use the basic ring (ring_impl_type=\"basic\", ring_flash_attn_func), which serves "
                                  "it over global positions with USP_RING_ALIBI=global")


def _check_dropout(dropout_p, q, softcap, alibi_slopes, group, packed, served, served_beyond_one_block):
    """Dropout (flash-attn's dropout_p) on a ring: the drop probability as the block launches take it, or None when it is off.
    The mask is a function of global positions (include/usp_hip.h: usp_flash_fwd_dropout), so a ring serves it where it places
    every block in the whole sequence: the dense rings at ring degree 1 (ONE block: basic, zigzag, stripe) and the basic ring
    beyond (`served_beyond_one_block`), by default; `served` = False: a ring whose forward takes no rng_state -- the reference has no competing semantics there (its ring backward drops
    the rng state).  Everything else refuses; NaN, a negative value or one >= 1 is a ValueError (_C.dropout_value).
    _check_hot_path_args still refuses dropout for every caller that does not come through here (the async layer)."""
    p = dropout_value(dropout_p)
    if p is None:
        return None
    if packed:
        raise NotImplementedError("dropout_p != 0 is not supported by the variable-length (packed) rings: use the basic ring "
                                  "(ring_impl_type=\"basic\", ring_flash_attn_func) on dense batches")
    if not served:
        raise NotImplementedError("dropout_p != 0 is not supported by this HIP ring attention: use the basic ring "
                                  "(ring_impl_type=\"basic\", ring_flash_attn_func)")
    if softcap_value(softcap) is not None:
        raise NotImplementedError("dropout_p together with softcap is not supported by the HIP attention kernels")
    if alibi_slopes is not None:
        raise NotImplementedError("dropout_p together with alibi_slopes is not supported by the HIP attention kernels")
    P = group_info(dist, group)[0]
    if P > 1 and not served_beyond_one_block:
        raise NotImplementedError("dropout_p != 0 across ring steps (ring degree > 1) is not supported by the zigzag and stripe "
                                  "rings: use the basic ring (ring_impl_type=\"basic\", ring_flash_attn_func), which serves it "
                                  "over global positions")
    if P > 1 and q.shape[1] % 4:
        raise NotImplementedError(f"dropout_p != 0 at ring degree {P} needs a local sequence length that is a multiple of 4 "
                                  f"(one Philox call covers a 4 x 4 patch of the mask), got {q.shape[1]}")
    return p


def _check_sinks(sinks, q, dropout_p, softcap, alibi_slopes, packed):
    """Attention sinks (one learned logit per query head, include/usp_hip.h: usp_flash_fwd_sink) on a ring.  The sink is
    position-free and counts once per row, and every dense ring opens each row's running state with exactly one launch without
    merge_in: the sink rides on that launch (kernels/attention.py: _SinkBackend), at any ring degree, and the merges and the
    backward kernels are unchanged.  The packed rings refuse, and so does a second score-level step (softcap, alibi_slopes,
    dropout_p); a wrong shape, dtype or device is a ValueError (_C.sinks_value)."""
    if sinks is None:
        return
    if packed:
        raise NotImplementedError("sinks is not supported by the variable-length (packed) rings: use a dense ring "
                                  "(ring_flash_attn_func, zigzag_ring_flash_attn_func, stripe_flash_attn_func)")
    for on, what in ((softcap_value(softcap) is not None, "softcap"), (alibi_slopes is not None, "alibi_slopes"),
                     (dropout_value(dropout_p) is not None, "dropout_p")):
        if on:
            raise NotImplementedError(f"sinks together with {what} is not supported by the HIP attention kernels")
    sinks_value(sinks, q.shape[2], q.device, q.dtype)


def _check_doc(cu_doclens, q, k, causal, window_size, softcap, alibi_slopes, dropout_p, sinks, group, packed, served_beyond_one_block):
    """The document mask (`cu_doclens`, ring/doc_blocks.py) on a ring: the parsed lists, or None when it is off or names one
    document (exactly the call without it).  `cu_doclens` describes the WHOLE sequence, ring degree x the local length, and is
    the same on every rank.  Served by the basic ring at any ring degree and by the zigzag and stripe rings at ring degree 1,
    where they are one block over the natural order; the packed rings refuse.  causal=False, whole q and k of different lengths
    and a second mask or score-level step beside it are refused; a malformed list is a ValueError."""
    if cu_doclens is None:
        return None
    if packed:
        raise NotImplementedError("cu_doclens is not supported by the variable-length (packed) rings: use LongContextAttention "
                                  "(ring_impl_type=\"basic\") or ring_flash_attn_func on dense batches")
    P = group_info(dist, group)[0]
    docs = doc_blocks.parse(cu_doclens, q.shape[0], P * q.shape[1])
    doc_blocks.refuse_not_causal_self(causal, P * q.shape[1], P * k.shape[1])
    window = None if window_size is None or tuple(window_size) == (-1, -1) else tuple(window_size)
    doc_blocks.refuse_beside(window, softcap_value(softcap), alibi_slopes, dropout_value(dropout_p), sinks)
    if docs is doc_blocks.SINGLE:
        return None
    if P > 1 and not served_beyond_one_block:
        raise NotImplementedError("cu_doclens across ring steps (ring degree > 1) is not supported by the zigzag and stripe "
                                  "rings: use the basic ring (ring_impl_type=\"basic\", ring_flash_attn_func)")
    return docs


def _basic_ring():
    """The basic ring's (forward, backward): what a one-block zigzag or stripe call under a document mask runs (at ring degree 1
    every dense ring is one block over the natural order)."""
    from .ring_flash_attn import ring_flash_attn_backward, ring_flash_attn_forward
    return ring_flash_attn_forward, ring_flash_attn_backward


def ring_dropout(dropout_p, rng_state):
    """(p, seed, head0) as get_block_backend takes it, from a ring forward's / backward's `dropout_p` and `rng_state` =
    (seed, head0); None when dropout is off.  dropout_p > 0 without a state is a caller that did not come through the front
    end: refused, as ever."""
    p = dropout_value(dropout_p)
    if p is None:
        return None
    if rng_state is None:
        raise NotImplementedError("dropout_p != 0 is not supported by the HIP ring attention without rng_state=(seed, head0) "
                                  "(the ring's *_func draw one per call)")
    return p, int(rng_state[0]), int(rng_state[1])


def ring_front_end(stem, class_name, forward, backward, packed=False, attn_processor=False, window_in_forward=False,
                   alibi_in_forward=False, dropout=False, dropout_in_forward=False, sinks=False, doc=False):
    """(Function, <stem>_func, <stem>_kvpacked_func, <stem>_qkvpacked_func) of the ring `forward` / `backward`.

        packed             the variable-length form: q / k / v are (T, H, D) token tensors followed by `cu_seqlens, max_seqlen`;
                           k and v are made contiguous (the dense form takes any view the kernels can address, kernel_operand),
                           there is no `attn_type`, and `return_attn_probs` hands the flattened (H, T) LSE back in the
                           reference's padded (num_seq, H, max_seqlen) layout;
        attn_processor     the Function carries `attn_processor` to the forward (the basic ring);
        window_in_forward  `window_size` is judged by the forward, not here (the basic ring serves a window at ring degree 1
                           and refuses beyond);
        alibi_in_forward   `alibi_slopes` at ring degree > 1 is judged by the forward (the basic ring: USP_RING_ALIBI); every
                           other dense ring serves it at ring degree 1, where it is one block, and refuses beyond; the packed
                           rings refuse it (_check_alibi);
        dropout            `forward` / `backward` take `rng_state=(seed, head0)` and serve `dropout_p` at ring degree 1 (every
                           dense ring); dropout_in_forward: also beyond (the basic ring).  One seed per call is drawn here from
                           torch's default CPU generator (draw_seed), in the autograd forward, and reused by the backward; the
                           dense *_func take the keyword-only `dropout_head0` (the global index of the call's query head 0: the
                           Ulysses layers pass their rank's), the Function an optional trailing argument of that name;
        sinks              `forward` takes `sinks=` and `backward` takes it too and returns (dq, dk, dv, dsinks fp32) with it (the
                           dense rings, any ring degree: _check_sinks).  The dense *_func take the keyword-only `sinks`, (Hq,)
                           fp32 or q.dtype, which may require grad; the Function takes it as one more optional trailing
                           argument (behind dropout_head0) and its backward returns the gradient in that slot, in the sinks'
                           dtype.  It is THIS rank's share -- its rows; the sum over the ring group is the gradient of the
                           replicated parameter, and nothing here reduces it.
        doc                `forward` / `backward` take `cu_doclens=` (the parsed lists) and serve the document mask at any ring
                           degree (the basic ring).  Every dense *_func takes the keyword-only `cu_doclens` (_check_doc); a ring
                           without `doc` serves it at ring degree 1 by the basic ring's one-block call and refuses beyond.  The
                           Function takes it as one more optional trailing argument (behind sinks).
    The dense <stem>_func pads head dims the kernels do not instantiate and skips the autograd node when nothing requires
    grad; both exist here only."""
    n_lead = 2 if packed else 0
    extra = () if packed else (("attn_type", "attn_processor") if attn_processor else ("attn_type",))
    n_args = n_lead + 9 + len(extra)

    def ring_pair(docs):
        """The (forward, backward) that run a call: this ring's, or -- under a document mask on a ring without `doc`, which
        _check_doc lets through at ring degree 1 only -- the basic ring's one-block call."""
        return (forward, backward) if doc or docs is None else _basic_ring()

    def run_forward(q, k, v, lead, dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes, group, extra_kw,
                    head0=0, sink_t=None, cu_doc=None):
        """Checks, operands, the ring forward: (the operands as launched, the scale used, out, lse, the dropout keywords of the
        backward)."""
        if softmax_scale is None:
            softmax_scale = q.shape[-1] ** (-0.5)
        if sink_t is not None:
            assert sinks, f"{class_name}: this ring's forward takes no sinks"
            _check_sinks(sink_t, q, dropout_p, softcap, alibi_slopes, packed)
        docs = _check_doc(cu_doc, q, k, causal, window_size, softcap, alibi_slopes, dropout_p, sink_t, group, packed, doc)
        _check_alibi(alibi_slopes, q, softcap, group, packed, alibi_in_forward)
        p = _check_dropout(dropout_p, q, softcap, alibi_slopes, group, packed, dropout, dropout_in_forward)
        _check_hot_path_args(dropout_p if p is None else 0.0, (-1, -1) if window_in_forward else window_size, softcap)
        if packed:
            k, v = k.contiguous(), v.contiguous()
        else:
            q, k, v = kernel_operand(q), kernel_operand(k), kernel_operand(v)     # any view a caller holds (maybe_contiguous)
        drop_kw = {} if p is None else dict(rng_state=(draw_seed(), int(head0)))  # one seed per call, host side
        if docs is not None:                      # (kept with the backward's keywords: drop_kw is what the backward adds)
            drop_kw = dict(drop_kw, cu_doclens=docs)
        ring_forward = ring_pair(docs)[0]
        out, lse = ring_forward(group, q, k, v, *lead, softmax_scale=softmax_scale, dropout_p=dropout_p, causal=causal,
                                window_size=window_size, softcap=softcap, alibi_slopes=alibi_slopes, deterministic=False, **extra_kw,
                                **drop_kw, **({} if sink_t is None else dict(sinks=sink_t)))
        return q, k, v, softmax_scale, out, lse, drop_kw

    def result(out, lse, lead, return_softmax):
        if not return_softmax:
            return out
        return out, (unflatten_lse(lse, *lead) if packed else lse), None

    class Func(torch.autograd.Function):
        """forward(ctx, q, k, v, [cu_seqlens, max_seqlen,] dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes,
        deterministic, return_softmax, group[, attn_type[, attn_processor]][, dropout_head0[, sinks]])"""

        @staticmethod
        def forward(ctx, q, k, v, *args):
            assert len(args) in (n_args, n_args + 1, n_args + 2, n_args + 3), \
                f"{class_name}: {n_args + 3} arguments expected (+ dropout_head0 (+ sinks (+ cu_doclens)))"
            ctx.n_none = len(args)
            head0 = args[n_args] if len(args) > n_args else 0
            sink_t = args[n_args + 1] if len(args) > n_args + 1 else None
            cu_doc = args[n_args + 2] if len(args) > n_args + 2 else None
            lead, extra_kw = args[:n_lead], dict(zip(extra, args[n_lead + 9:n_args]))
            dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes, deterministic, return_softmax, group = \
                args[n_lead:n_lead + 9]
            q, k, v, softmax_scale, out, lse, drop_kw = run_forward(q, k, v, lead, dropout_p, softmax_scale, causal, window_size,
                                                                    softcap, alibi_slopes, group, extra_kw, head0, sink_t, cu_doc)
            ctx.has_sinks = sink_t is not None                                    # (dense rings only: `lead` is then empty)
            ctx.save_for_backward(q, k, v, out, lse, *lead[:1], *(() if sink_t is None else (sink_t,)))   # (cu_seqlens is a tensor)
            extra_kw.pop("attn_processor", None)                                  # (the backwards take none)
            ctx.call = (group, lead[1:], dict(softmax_scale=softmax_scale, dropout_p=dropout_p, causal=causal,
                                              window_size=window_size, softcap=softcap, alibi_slopes=alibi_slopes,
                                              deterministic=deterministic, **extra_kw, **drop_kw))
            return result(out, lse, lead, return_softmax)

        @staticmethod
        def backward(ctx, dout, *args):
            group, lead_rest, kw = ctx.call
            if not packed:
                dout = kernel_operand(dout)
            if not ctx.has_sinks:
                ring_backward = ring_pair(kw.get("cu_doclens"))[1]
                return tuple(ring_backward(group, dout, *ctx.saved_tensors, *lead_rest, **kw)) + (None,) * ctx.n_none
            *saved, sink_t = ctx.saved_tensors
            dq, dk, dv, dsinks = backward(group, dout, *saved, *lead_rest, **kw, sinks=sink_t)
            return (dq, dk, dv) + (None,) * (ctx.n_none - 1) + (dsinks.to(sink_t.dtype),)

    Func.__name__ = Func.__qualname__ = class_name

    if packed:
        def func(q, k, v, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1),
                 softcap=0.0, alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None, *, sinks=None,
                 cu_doclens=None):
            _check_doc(cu_doclens, q, k, causal, window_size, softcap, alibi_slopes, dropout_p, sinks, group, packed, doc)
            _check_sinks(sinks, q, dropout_p, softcap, alibi_slopes, packed)
            return Func.apply(q, k, v, cu_seqlens, max_seqlen, dropout_p, softmax_scale, causal, window_size, softcap,
                              alibi_slopes, deterministic, return_attn_probs, group)

        def kvpacked_func(q, kv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
                          window_size=(-1, -1), softcap=0.0, alibi_slopes=None, deterministic=False, return_attn_probs=False,
                          group=None, *, sinks=None, cu_doclens=None):
            _check_doc(cu_doclens, q, kv[:, 0], causal, window_size, softcap, alibi_slopes, dropout_p, sinks, group, packed, doc)
            _check_sinks(sinks, q, dropout_p, softcap, alibi_slopes, packed)
            return Func.apply(q, kv[:, 0], kv[:, 1], cu_seqlens, max_seqlen, dropout_p, softmax_scale, causal, window_size,
                              softcap, alibi_slopes, deterministic, return_attn_probs, group)

        def qkvpacked_func(qkv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
                           window_size=(-1, -1), softcap=0.0, alibi_slopes=None, deterministic=False, return_attn_probs=False,
                           group=None, *, sinks=None, cu_doclens=None):
            _check_doc(cu_doclens, qkv[:, 0], qkv[:, 1], causal, window_size, softcap, alibi_slopes, dropout_p, sinks, group, packed, doc)
            _check_sinks(sinks, qkv[:, 0], dropout_p, softcap, alibi_slopes, packed)
            return Func.apply(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu_seqlens, max_seqlen, dropout_p, softmax_scale, causal,
                              window_size, softcap, alibi_slopes, deterministic, return_attn_probs, group)
    else:
        def last(attn_type, processor=None):      # the Function's trailing arguments
            return (attn_type, processor)[:len(extra)]

        def head0_arg(dropout_head0, sink_t=None, cu_doc=None):    # ... and the optional ones behind them
            if cu_doc is not None:
                return (dropout_head0, sink_t, cu_doc)
            return (dropout_head0, sink_t) if sink_t is not None else ((dropout_head0,) if dropout_head0 else ())

        def func(q, k, v, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                 alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None,
                 attn_type: AttnType = AttnType.HIP, attn_processor=None, *, dropout_head0=0, sinks=None, cu_doclens=None):
            D = q.shape[-1]
            if kernel_head_dim(D) != D:      # a head dim the kernels do not instantiate (e.g. 96): zero-padded copies
                res = func(*pad_head_dim(q, k, v), dropout_p, D ** -0.5 if softmax_scale is None else softmax_scale, causal,
                           window_size, softcap, alibi_slopes, deterministic, return_attn_probs, group, attn_type, attn_processor,
                           dropout_head0=dropout_head0, sinks=sinks, cu_doclens=cu_doclens)
                return (res[0][..., :D],) + tuple(res[1:]) if isinstance(res, tuple) else res[..., :D]
            if not needs_grad(q, k, v, *(() if sinks is None else (sinks,))):      # inference / forward-only benchmarks: no autograd node, no saved tensors (~25 us)
                out, lse = run_forward(q, k, v, (), dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes, group,
                                       dict(zip(extra, last(attn_type, attn_processor))), dropout_head0, sinks, cu_doclens)[4:6]
                return result(out, lse, (), return_attn_probs)
            return Func.apply(q, k, v, dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes, deterministic,
                              return_attn_probs, group, *last(attn_type, attn_processor), *head0_arg(dropout_head0, sinks, cu_doclens))

        def kvpacked_func(q, kv, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                          alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None,
                          attn_type: AttnType = AttnType.HIP, *, dropout_head0=0, sinks=None, cu_doclens=None):
            return Func.apply(q, kv[:, :, 0], kv[:, :, 1], dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes,
                              deterministic, return_attn_probs, group, *last(attn_type), *head0_arg(dropout_head0, sinks, cu_doclens))

        def qkvpacked_func(qkv, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                           alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None,
                           attn_type: AttnType = AttnType.HIP, *, dropout_head0=0, sinks=None, cu_doclens=None):
            return Func.apply(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], dropout_p, softmax_scale, causal, window_size, softcap,
                              alibi_slopes, deterministic, return_attn_probs, group, *last(attn_type),
                              *head0_arg(dropout_head0, sinks, cu_doclens))

    for fn, suffix in ((func, "_func"), (kvpacked_func, "_kvpacked_func"), (qkvpacked_func, "_qkvpacked_func")):
        fn.__name__ = fn.__qualname__ = stem + suffix
    return Func, func, kvpacked_func, qkvpacked_func
