"""The public front end of every ring: ONE autograd Function and ONE *_func / *_kvpacked_func / *_qkvpacked_func trio,
made per ring from its (forward, backward) pair.  The ring modules keep their schedules and bind their public names to what
`ring_front_end` returns; the surfaces are the reference's (yunchang/ring/*.py), argument for argument."""
from typing import NamedTuple

import torch
import torch.distributed as dist

from .._C import BLOCK_SELECT_MAX_BLOCKS, block_select_top_p_value, block_select_value, dropout_value, softcap_value
from ..kernels import AttnType
from ..kernels.attention import (block_attention_mass, draw_seed, get_block_backend, kernel_head_dim, kernel_operand,
                                 mass_operands, needs_grad, pad_head_dim, select_blocks, select_blocks_top_p, select_operands)
from ..kernels.features import (BLOCK_MASK_SIZE, BlockSelectTopP, Features, block_mask_alone, block_mask_self_attention, block_select_alone,
                                max_logits_alone, return_block_mass_alone)
from .utils import RingComm, group_info
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


NOT_SERVED, ONE_BLOCK, ANY_DEGREE = 0, 1, 2


class RingServes(NamedTuple):
    """What one ring serves of the features whose block launches depend on where the block lies (kernels/features.py), each
    NOT_SERVED, ONE_BLOCK (at ring degree 1, where every dense ring is one block over the natural order) or ANY_DEGREE (the
    ring's forward places every block, or refuses by its own rules: the basic ring's USP_RING_WINDOW / USP_RING_ALIBI).  With
    it goes what `forward` / `backward` take: `rng_state=(seed, head0)` where dropout is served, `sinks=` where sinks are (the
    backward then returns (dq, dk, dv, dsinks fp32)), `cu_doclens=` (the parsed lists) where the document mask is served at
    ANY_DEGREE -- a ring with ONE_BLOCK there hands such a call to the basic ring's one-block call.  ONE_BLOCK has a meaning for
    alibi, dropout and doc only: a window is either left to the ring's forward (ANY_DEGREE) or refused, and the sinks, being
    position-free, are served at any degree or not at all (ring_front_end asserts both)."""
    window: int = NOT_SERVED
    alibi: int = NOT_SERVED
    dropout: int = NOT_SERVED
    sinks: int = NOT_SERVED
    doc: int = NOT_SERVED
    span: int = NOT_SERVED        # bidirectional spans: they ride inside the parsed `cu_doclens` plan (ring/doc_blocks.py: Spans)
    block_mask: int = NOT_SERVED  # a 128 x 128 block mask: it rides in the `cu_doclens` slot as a BlockMask (below); ANY_DEGREE:
                                  # the ring's forward / backward hand every (rank, step) launch its view of it (`bsp=`)
    max_logits: int = NOT_SERVED  # return_max_logits: row-local and position-free like the sinks, so ANY_DEGREE or not at all; the
                                  # ring's forward takes `max_logits=True` and returns (out, lse, this rank's share fp32 (Hq,))


PACKED_RING = RingServes()
DENSE_RING = RingServes(alibi=ONE_BLOCK, dropout=ONE_BLOCK, sinks=ANY_DEGREE, doc=ONE_BLOCK, span=ONE_BLOCK,
                        block_mask=ONE_BLOCK, max_logits=ANY_DEGREE)                                                                    # zigzag, stripe
BASIC_RING = RingServes(*(ANY_DEGREE,) * 8)

# feature -> (its name in the refusals, what the packed rings advise, what a ONE_BLOCK ring advises beyond ring degree 1)
_BASIC = "use the basic ring (ring_impl_type=\"basic\", ring_flash_attn_func)"
_ADVICE = {
    "doc": ("cu_doclens", "use LongContextAttention (ring_impl_type=\"basic\") or ring_flash_attn_func on dense batches", _BASIC),
    "span": ("bidirectional", "use LongContextAttention (ring_impl_type=\"basic\") or ring_flash_attn_func on dense batches", _BASIC),
    "sinks": ("sinks", "use a dense ring (ring_flash_attn_func, zigzag_ring_flash_attn_func, stripe_flash_attn_func)", None),
    "alibi": ("alibi_slopes", _BASIC + " on dense batches", _BASIC + ", which serves it over global positions with "
                                                                      "USP_RING_ALIBI=global"),
    "dropout": ("dropout_p != 0", _BASIC + " on dense batches", _BASIC + ", which serves it over global positions"),
}


def _refuse_unserved(serves, doc=None, sinks=None, alibi=None, dropout=None):
    """NOT_SERVED is what the packed rings are: the first of the given ones that is on and not served is refused in their name."""
    for feature, value in (("doc", doc), ("sinks", sinks), ("alibi", alibi), ("dropout", dropout)):
        if feature == "doc" and _has_spans(value):
            feature = "span"
        if value is not None and not getattr(serves, feature):
            name, advice, _ = _ADVICE[feature]
            raise NotImplementedError(f"{name} is not supported by the variable-length (packed) rings: {advice}")


def _has_spans(docs) -> bool:
    return getattr(docs, "spans", None) is not None


def span_plan(q, group, cu_doclens, bidirectional):
    """`cu_doclens` for the rest of a ring call that was given `bidirectional`: the parsed plan with the spans inside
    (ring/doc_blocks.py: parse_plan, over the WHOLE sequence: ring degree x the local length), or `cu_doclens` as given where the
    spans are off -- None, an empty list, spans of length 1 only: exactly the call without the keyword."""
    if bidirectional is None:
        return cu_doclens
    from . import doc_blocks
    plan = doc_blocks.parse_plan(cu_doclens, bidirectional, q.shape[0], group_info(dist, group)[0] * q.shape[1])
    return plan if _has_spans(plan) else cu_doclens


def _span_given(bidirectional) -> bool:
    """Is `bidirectional` anything but None or an empty list?  (What the packed rings, which hold no whole sequence to parse
    it against, refuse.)"""
    if bidirectional is None:
        return False
    try:
        return isinstance(bidirectional, str) or len(bidirectional) > 0
    except TypeError:
        return True


def _refuse_packed_spans(bidirectional):
    if _span_given(bidirectional):
        name, advice, _ = _ADVICE["span"]
        raise NotImplementedError(f"{name} is not supported by the variable-length (packed) rings: {advice}")


class BlockMask:
    """The `block_mask` of a dense ring call on its way to the ring's forward / backward: it travels in the `cu_doclens` slot
    (with which it never goes together), so the Function keeps its arguments.  `mask` covers the WHOLE sequence -- ring degree x
    the local length -- and is the same on every rank; it is a device tensor and is never read on the host.
    `rows_only` (what a ring rank SELECTS under `block_select=`: select_block_rows): `mask` (B, Hq, n, nb) holds this rank's n
    row blocks against the key blocks of the whole sequence -- a whole (nb, nb) mask is never made."""
    spans = None

    def __init__(self, mask, rows_only: bool = False):
        self.mask, self.rows_only = mask, bool(rows_only)

    def view(self, r: int, kr: int, S: int, P: int):
        """The sub-mask of the launch of rank r's rows [r S, (r + 1) S) against ring rank kr's keys: a strided view, no copy."""
        if P == 1:
            return self.mask
        n = S // BLOCK_MASK_SIZE
        if self.rows_only:
            return self.mask[..., kr * n:(kr + 1) * n]
        return self.mask[..., r * n:(r + 1) * n, kr * n:(kr + 1) * n]


class BlockSelection:
    """The `block_select` of a dense ring call on its way to the ring's forward: like a BlockMask it rides in the `cu_doclens`
    slot, and run_forward turns it into the BlockMask it selects -- once: the backward gets that mask."""
    spans = None

    def __init__(self, select):
        self.select = select


def _refuse_packed_block_select(block_select):
    if block_select is not None:
        raise NotImplementedError("block_select is not supported by the variable-length (packed) rings: use LongContextAttention "
                                  "(ring_impl_type=\"basic\") or ring_flash_attn_func on dense batches")


def _refuse_packed_block_mask(block_mask):
    if block_mask is not None:
        raise NotImplementedError("block_mask is not supported by the variable-length (packed) rings: use LongContextAttention "
                                  "(ring_impl_type=\"basic\") or ring_flash_attn_func on dense batches")


def _refuse_packed_max_logits(return_max_logits):
    if return_max_logits:
        raise NotImplementedError("return_max_logits is not supported by the variable-length (packed) rings: use a dense ring "
                                  "(ring_flash_attn_func, zigzag_ring_flash_attn_func, stripe_flash_attn_func)")


def _refuse_packed_block_mass(return_block_mass):
    if return_block_mass:
        raise NotImplementedError("return_block_mass is not supported by the variable-length (packed) rings: use "
                                  "LongContextAttention (ring_impl_type=\"basic\") or ring_flash_attn_func on dense batches")


def ring_block_attention_mass(q, k, lse, *, softmax_scale=None, causal=False, group=None):
    """The block-pooled attention map (kernels/attention.py: block_attention_mass) of the BASIC ring, this rank's share: rank r of
    ring degree P holds the rows [r S, (r + 1) S) of the whole sequence (q (B, S, Hq, D), k (B, S, Hkv, D), and the ring's lse
    (B, Hq, S) of those rows -- what ring_flash_attn_func(..., return_attn_probs=True) returns) and gets the rows-only share
    fp32 (B, Hq, n, nb), n = S / 128 row blocks against all nb = P n key blocks: the coordinates of a ring rank's selected mask
    (select_block_rows), so block_mask_recall takes both.  The shares of the ranks, stacked along the row-block dim in rank
    order, are the single-device map bit for bit.  K alone makes the ring's rotation -- P - 1 hops, no V: step s holds the keys
    of ring rank kr = r - s (mod P) and writes the column slice [kr n, (kr + 1) n) with the diagonal s * S
    (include/usp_hip.h: usp_block_attn_mass).  Under `causal` the steps s > r launch nothing and their slices stay zero.  No
    gradient, nothing read on the host.  Ring degree 1: block_attention_mass.  NotImplementedError: q and k of different
    lengths, a local length that is no multiple of 128 at ring degree > 1."""
    P, r = group_info(dist, group)
    if P == 1:
        return block_attention_mass(q, k, lse, softmax_scale=softmax_scale, causal=causal)
    block_mask_self_attention(q.shape[1], k.shape[1], "ring_block_attention_mass")
    S = q.shape[1]
    if S % BLOCK_MASK_SIZE:
        raise NotImplementedError(f"ring_block_attention_mass at ring degree {P} needs a local sequence length that is a multiple "
                                  f"of {BLOCK_MASK_SIZE} (whole blocks per rank), got {S}: pad the sequence")
    q, k, lse, scale = mass_operands(q, k, lse, softmax_scale)
    n = S // BLOCK_MASK_SIZE
    make = torch.zeros if causal else torch.empty        # (causal: the slices of the steps that launch nothing stay zero)
    mass = make((q.shape[0], q.shape[2], n, P * n), dtype=torch.float32, device=q.device)
    be = get_block_backend()
    kk = k.contiguous()
    for step in range(P):
        comm = nxt = None
        if step + 1 < P:                                 # K alone travels: P - 1 hops
            comm = RingComm(group)
            nxt = comm.send_recv(kk)
            comm.commit()
        if not causal or step <= r:
            kr = (r - step) % P
            be.block_mass(q, kk, lse, scale, bool(causal), step * S, mass[..., kr * n:(kr + 1) * n])
        if comm is not None:
            comm.wait()
            kk = nxt
    return mass


def block_mass_call(serves, call, q, k, softmax_scale, causal, group, return_attn_probs):
    """A dense ring call under `return_block_mass` (judged alone already: nothing else is on): `call(return_attn_probs=True)` --
    the call without the keyword, bit for bit -- and behind it the rank's share of the map from the call's own lse
    (ring_block_attention_mass).  The zigzag and stripe rings hold other rows than the basic ring's slices: they serve ring
    degree 1."""
    P = group_info(dist, group)[0]
    if P > 1 and serves.block_mask != ANY_DEGREE:
        raise NotImplementedError(f"return_block_mass across ring steps (ring degree > 1) is not supported by the zigzag and "
                                  f"stripe rings: {_BASIC}")
    block_mask_self_attention(q.shape[1], k.shape[1], "return_block_mass")
    if P > 1 and q.shape[1] % BLOCK_MASK_SIZE:
        raise NotImplementedError(f"return_block_mass at ring degree {P} needs a local sequence length that is a multiple of "
                                  f"{BLOCK_MASK_SIZE} (whole blocks per rank), got {q.shape[1]}: pad the sequence")
    out, lse, _ = call(True)
    mass = ring_block_attention_mass(q, k, lse, softmax_scale=softmax_scale, causal=causal, group=group)
    return (out, lse, None, mass) if return_attn_probs else (out, mass)


def block_mask_plan(block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional, block_select=None):
    """`cu_doclens` for the rest of a dense ring call: the BlockMask where `block_mask` is given -- judged first, alone
    (kernels/features.py: block_mask_alone) --, the BlockSelection where `block_select` is (block_select_alone), else
    `cu_doclens` as it is."""
    if block_select_alone(block_select, block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional):
        return BlockSelection(block_select)
    if block_mask_alone(block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional):
        return BlockMask(block_mask)
    return cu_doclens


def _place_block_mask(serves, q, k, bm, group):
    """The checks of a ring call under a block mask: what this ring serves, whole blocks per rank, the value itself."""
    from .._C import block_mask_value
    P = group_info(dist, group)[0]
    if P > 1 and serves.block_mask != ANY_DEGREE:
        raise NotImplementedError(f"block_mask across ring steps (ring degree > 1) is not supported by the zigzag and stripe "
                                  f"rings: {_BASIC}")
    block_mask_self_attention(q.shape[1], k.shape[1])
    if P > 1 and q.shape[1] % BLOCK_MASK_SIZE:
        raise NotImplementedError(f"block_mask at ring degree {P} needs a local sequence length that is a multiple of "
                                  f"{BLOCK_MASK_SIZE} (whole mask blocks per rank), got {q.shape[1]}: pad the sequence")
    block_mask_value(bm.mask, q.shape[0], q.shape[2], P * q.shape[1], q.device)


def _place_block_select(serves, q, k, sel, causal, group):
    """The checks of a ring call under a block selection: those of a block mask, in its name, and the selection's own."""
    P = group_info(dist, group)[0]
    if P > 1 and serves.block_mask != ANY_DEGREE:
        raise NotImplementedError(f"block_select across ring steps (ring degree > 1) is not supported by the zigzag and stripe "
                                  f"rings: {_BASIC}")
    block_mask_self_attention(q.shape[1], k.shape[1], "block_select")
    if P > 1 and q.shape[1] % BLOCK_MASK_SIZE:
        raise NotImplementedError(f"block_select at ring degree {P} needs a local sequence length that is a multiple of "
                                  f"{BLOCK_MASK_SIZE} (whole mask blocks per rank), got {q.shape[1]}: pad the sequence")
    if isinstance(sel.select, BlockSelectTopP):
        block_select_top_p_value(*sel.select, causal)
    else:
        block_select_value(*sel.select, causal)


def select_block_rows(q, k, select, softmax_scale, causal, group):
    """The BlockMask a ring rank runs under `block_select`: kernels/attention.py: select_blocks over the WHOLE sequence,
    restricted to this rank's rows.  Ring degree 1: the whole mask.  Beyond: the rank pools its own q and k slices (n =
    S_local / 128 blocks each), all-gathers the pooled keys -- fp32 (B, n, Hkv, D), ONE all_gather_into_tensor per call -- and
    selects its n row blocks, the first of them the global block r * n, against all nb key blocks: a rows-only mask
    (B, Hq, n, nb).  Nothing is read on the host.  A BlockSelectTopP runs the same scheme through select_blocks_top_p /
    block_select_top_p (a rank of the ring holds every head, so share_group needs nothing more)."""
    P, r = group_info(dist, group)
    top_p = isinstance(select, BlockSelectTopP)
    if top_p:
        p, keep_first, keep_local, share = block_select_top_p_value(*select, causal)
        if P == 1:
            return BlockMask(select_blocks_top_p(q, k, p, softmax_scale=softmax_scale, causal=causal, keep_first=keep_first,
                                                 keep_local=keep_local, share_group=share))
    else:
        top_k, keep_first, keep_local = block_select_value(*select, causal)
    if P == 1:
        return BlockMask(select_blocks(q, k, top_k, softmax_scale=softmax_scale, causal=causal, keep_first=keep_first,
                                       keep_local=keep_local))
    qs, ks, scale = select_operands(q, k, softmax_scale)
    be = get_block_backend()
    qbar, kbar_local = be.block_means(qs), be.block_means(ks)
    B, n, Hkv, D = kbar_local.shape
    if P * n > BLOCK_SELECT_MAX_BLOCKS:
        raise NotImplementedError(f"block_select serves up to {BLOCK_SELECT_MAX_BLOCKS} blocks of {BLOCK_MASK_SIZE} keys, got {P * n}")
    gathered = torch.empty((P * B, n, Hkv, D), dtype=torch.float32, device=kbar_local.device)
    dist.all_gather_into_tensor(gathered, kbar_local.contiguous(), group=group)
    kbar = gathered.view(P, B, n, Hkv, D).permute(1, 0, 2, 3, 4).reshape(B, P * n, Hkv, D)   # (rank-major -> the global order)
    if top_p:
        return BlockMask(be.block_select_top_p(qbar, kbar.contiguous(), p, scale, bool(causal), keep_first, keep_local, share, r * n),
                         rows_only=True)
    return BlockMask(be.block_select(qbar, kbar.contiguous(), top_k, scale, bool(causal), keep_first, keep_local, r * n), rows_only=True)


def _place(serves, q, k, causal, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, group):
    """(the drop probability, the parsed document lists) of one ring call, None = off, or the refusal of what this ring does not
    serve or the kernels do not serve together (kernels/features.py: Features).
    The block launches of ALiBi, dropout and the document mask depend on where the block lies in the WHOLE sequence (ring degree
    x the local length; `cu_doclens` describes all of it and is the same on every rank), so a ring serves them only where it
    places every block; the sink is position-free and rides on the one launch without merge_in with which every dense ring opens
    a row range, at any ring degree.  For each feature that is on: the packed rings refuse, every dense ring serves ring degree
    1, beyond it only a ring that declares so (`serves`).  Then the combination table; a malformed value is a ValueError
    (Features.of).  A window that the ring's forward does not judge, and dropout from callers that do not come through here (the
    async layer), stay with _check_hot_path_args."""
    p = dropout_value(dropout_p)
    if cu_doclens is None and sinks is None and alibi_slopes is None and p is None:
        # the hot path: nothing to place, and nothing the table refuses (a window and softcap go with each other) -- no record
        _check_hot_path_args(dropout_p, (-1, -1) if serves.window else window_size, softcap)
        return None, None
    _refuse_unserved(serves, doc=cu_doclens, sinks=sinks, alibi=alibi_slopes, dropout=p)
    # (the ring degree is asked only where a feature needs it: a refusal by the table needs no process group)
    f = Features.of(q, k, causal, window_size, softcap, alibi_slopes, p, sinks, cu_doclens,
                    1 if cu_doclens is None else group_info(dist, group)[0])
    if f.doc is not None or f.alibi is not None or p is not None:
        P = group_info(dist, group)[0]
        for feature in ("doc", "alibi", "dropout"):
            key = "span" if feature == "doc" and _has_spans(f.doc) else feature
            if P > 1 and getattr(f, feature) is not None and getattr(serves, key) != ANY_DEGREE:
                name, _, advice = _ADVICE[key]
                raise NotImplementedError(f"{name} across ring steps (ring degree > 1) is not supported by the zigzag and stripe "
                                          f"rings: {advice}")
        if P > 1 and p is not None and q.shape[1] % 4:
            raise NotImplementedError(f"dropout_p != 0 at ring degree {P} needs a local sequence length that is a multiple of 4 "
                                      f"(one Philox call covers a 4 x 4 patch of the mask), got {q.shape[1]}")
    _check_hot_path_args(dropout_p if p is None else 0.0, (-1, -1) if serves.window else window_size, softcap)
    return p, f.doc


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


def ring_front_end(stem, class_name, forward, backward, serves: RingServes, packed=False, attn_processor=False):
    """(Function, <stem>_func, <stem>_kvpacked_func, <stem>_qkvpacked_func) of the ring `forward` / `backward`.

        serves             what the ring serves of window_size, alibi_slopes, dropout_p, sinks and cu_doclens, and with it what
                           `forward` / `backward` take (RingServes; the refusals: _place).
                           dropout: one seed per call is drawn here from torch's default CPU generator (draw_seed), in the
                           autograd forward, and reused by the backward; the dense *_func take the keyword-only `dropout_head0`
                           (the global index of the call's query head 0: the Ulysses layers pass their rank's), the Function an
                           optional trailing argument of that name.
                           sinks: the dense *_func take the keyword-only `sinks`, (Hq,) fp32 or q.dtype, which may require grad;
                           the Function takes it as one more optional trailing argument (behind dropout_head0) and its backward
                           returns the gradient in that slot, in the sinks' dtype.  It is THIS rank's share -- its rows; the sum
                           over the ring group is the gradient of the replicated parameter, and nothing here reduces it.
                           cu_doclens: every dense *_func takes the keyword-only `cu_doclens`; the Function takes it as one more
                           optional trailing argument (behind sinks).
        packed             the variable-length form: q / k / v are (T, H, D) token tensors followed by `cu_seqlens, max_seqlen`;
                           k and v are made contiguous (the dense form takes any view the kernels can address, kernel_operand),
                           there is no `attn_type`, and `return_attn_probs` hands the flattened (H, T) LSE back in the
                           reference's padded (num_seq, H, max_seqlen) layout;
        attn_processor     the Function carries `attn_processor` to the forward (the basic ring).
    The dense <stem>_func pads head dims the kernels do not instantiate and skips the autograd node when nothing requires
    grad; both exist here only."""
    assert ONE_BLOCK not in (serves.window, serves.sinks, serves.max_logits), \
        f"{class_name}: RingServes has no ONE_BLOCK for window, sinks and max_logits"
    n_lead = 2 if packed else 0
    extra = () if packed else (("attn_type", "attn_processor") if attn_processor else ("attn_type",))
    n_args = n_lead + 9 + len(extra)

    def ring_pair(docs):
        """The (forward, backward) that run a call: this ring's, or -- under a document mask on a ring that serves it as
        ONE_BLOCK, which _place lets through at ring degree 1 only -- the basic ring's one-block call.  `docs` is whatever rides
        in the `cu_doclens` slot: the parsed document plan, or a BlockMask (`block_mask=`; _place_block_mask lets it through
        beyond ring degree 1 on a ring with block_mask == ANY_DEGREE only) -- so a zigzag or stripe call under a block mask at
        ring degree 1 runs the basic ring's functions too."""
        return (forward, backward) if serves.doc == ANY_DEGREE or docs is None else _basic_ring()

    def run_forward(q, k, v, lead, dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes, group, extra_kw,
                    head0=0, sink_t=None, cu_doc=None, max_logits=False):
        """Checks, operands, the ring forward: (the operands as launched, the scale used, out, lse, the dropout keywords of the
        backward, this rank's share of the max logits | None).  `max_logits`: judged alone already (max_logits_alone): beside it
        only a window can be on, which the ring's forward judges or _check_hot_path_args refuses."""
        if softmax_scale is None:
            softmax_scale = q.shape[-1] ** (-0.5)
        if isinstance(cu_doc, BlockMask):           # (judged alone already: nothing else is on)
            _place_block_mask(serves, q, k, cu_doc, group)
            _check_hot_path_args(dropout_p, window_size, softcap)
            p, docs = None, cu_doc
        elif isinstance(cu_doc, BlockSelection):    # (likewise; the mask is selected below, from the operands as launched)
            _place_block_select(serves, q, k, cu_doc, causal, group)
            _check_hot_path_args(dropout_p, window_size, softcap)
            p, docs = None, cu_doc
        else:
            p, docs = _place(serves, q, k, causal, window_size, softcap, alibi_slopes, dropout_p, sink_t, cu_doc, group)
        if packed:
            k, v = k.contiguous(), v.contiguous()
        else:
            q, k, v = kernel_operand(q), kernel_operand(k), kernel_operand(v)     # any view a caller holds (maybe_contiguous)
        if isinstance(docs, BlockSelection):      # selected ONCE: the backward's keywords hold the mask (drop_kw below)
            docs = select_block_rows(q, k, docs.select, softmax_scale, causal, group)
        drop_kw = {} if p is None else dict(rng_state=(draw_seed(), int(head0)))  # one seed per call, host side
        if docs is not None:                      # (kept with the backward's keywords: drop_kw is what the backward adds)
            drop_kw = dict(drop_kw, cu_doclens=docs)
        ring_forward = ring_pair(docs)[0]
        out, lse, *ml = ring_forward(group, q, k, v, *lead, softmax_scale=softmax_scale, dropout_p=dropout_p, causal=causal,
                                     window_size=window_size, softcap=softcap, alibi_slopes=alibi_slopes, deterministic=False, **extra_kw,
                                     **drop_kw, **({} if sink_t is None else dict(sinks=sink_t)),
                                     **(dict(max_logits=True) if max_logits else {}))
        return q, k, v, softmax_scale, out, lse, drop_kw, (ml[0] if max_logits else None)

    def result(out, lse, lead, return_softmax, ml=None):
        """`out`, or `(out, lse, None)`; under return_max_logits `(out, max_logits)` or `(out, lse, None, max_logits)`."""
        tail = () if ml is None else (ml,)
        if not return_softmax:
            return (out,) + tail if tail else out
        return (out, (unflatten_lse(lse, *lead) if packed else lse), None) + tail

    class Func(torch.autograd.Function):
        """forward(ctx, q, k, v, [cu_seqlens, max_seqlen,] dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes,
        deterministic, return_softmax, group[, attn_type[, attn_processor]][, dropout_head0[, sinks[, cu_doclens[, max_logits]]]])"""

        @staticmethod
        def forward(ctx, q, k, v, *args):
            assert len(args) in (n_args, n_args + 1, n_args + 2, n_args + 3, n_args + 4), \
                f"{class_name}: {n_args + 3} arguments expected (+ dropout_head0 (+ sinks (+ cu_doclens (+ max_logits))))"
            ctx.n_none = len(args)
            head0 = args[n_args] if len(args) > n_args else 0
            sink_t = args[n_args + 1] if len(args) > n_args + 1 else None
            cu_doc = args[n_args + 2] if len(args) > n_args + 2 else None
            max_logits = bool(args[n_args + 3]) if len(args) > n_args + 3 else False
            lead, extra_kw = args[:n_lead], dict(zip(extra, args[n_lead + 9:n_args]))
            dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes, deterministic, return_softmax, group = \
                args[n_lead:n_lead + 9]
            q, k, v, softmax_scale, out, lse, drop_kw, ml = run_forward(q, k, v, lead, dropout_p, softmax_scale, causal, window_size,
                                                                        softcap, alibi_slopes, group, extra_kw, head0, sink_t, cu_doc,
                                                                        max_logits)
            if ml is not None:
                ctx.mark_non_differentiable(ml)                                   # (a statistic: the backward is untouched)
            ctx.has_sinks = sink_t is not None                                    # (dense rings only: `lead` is then empty)
            ctx.save_for_backward(q, k, v, out, lse, *lead[:1], *(() if sink_t is None else (sink_t,)))   # (cu_seqlens is a tensor)
            extra_kw.pop("attn_processor", None)                                  # (the backwards take none)
            ctx.call = (group, lead[1:], dict(softmax_scale=softmax_scale, dropout_p=dropout_p, causal=causal,
                                              window_size=window_size, softcap=softcap, alibi_slopes=alibi_slopes,
                                              deterministic=deterministic, **extra_kw, **drop_kw))
            return result(out, lse, lead, return_softmax, ml)

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
                 cu_doclens=None, bidirectional=None, block_mask=None, return_max_logits=False, block_select=None,
                 return_block_mass=False):
            _refuse_packed_block_mass(return_block_mass)
            _refuse_packed_max_logits(return_max_logits)
            _refuse_packed_block_mask(block_mask)
            _refuse_packed_block_select(block_select)
            _refuse_packed_spans(bidirectional)
            _refuse_unserved(serves, doc=cu_doclens, sinks=sinks)
            return Func.apply(q, k, v, cu_seqlens, max_seqlen, dropout_p, softmax_scale, causal, window_size, softcap,
                              alibi_slopes, deterministic, return_attn_probs, group)

        def kvpacked_func(q, kv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
                          window_size=(-1, -1), softcap=0.0, alibi_slopes=None, deterministic=False, return_attn_probs=False,
                          group=None, *, sinks=None, cu_doclens=None, bidirectional=None, block_mask=None, return_max_logits=False, block_select=None,
                 return_block_mass=False):
            _refuse_packed_block_mass(return_block_mass)
            _refuse_packed_max_logits(return_max_logits)
            _refuse_packed_block_mask(block_mask)
            _refuse_packed_block_select(block_select)
            _refuse_packed_spans(bidirectional)
            _refuse_unserved(serves, doc=cu_doclens, sinks=sinks)
            return Func.apply(q, kv[:, 0], kv[:, 1], cu_seqlens, max_seqlen, dropout_p, softmax_scale, causal, window_size,
                              softcap, alibi_slopes, deterministic, return_attn_probs, group)

        def qkvpacked_func(qkv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
                           window_size=(-1, -1), softcap=0.0, alibi_slopes=None, deterministic=False, return_attn_probs=False,
                           group=None, *, sinks=None, cu_doclens=None, bidirectional=None, block_mask=None, return_max_logits=False, block_select=None,
                 return_block_mass=False):
            _refuse_packed_block_mass(return_block_mass)
            _refuse_packed_max_logits(return_max_logits)
            _refuse_packed_block_mask(block_mask)
            _refuse_packed_block_select(block_select)
            _refuse_packed_spans(bidirectional)
            _refuse_unserved(serves, doc=cu_doclens, sinks=sinks)
            return Func.apply(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu_seqlens, max_seqlen, dropout_p, softmax_scale, causal,
                              window_size, softcap, alibi_slopes, deterministic, return_attn_probs, group)
    else:
        def last(attn_type, processor=None):      # the Function's trailing arguments
            return (attn_type, processor)[:len(extra)]

        def head0_arg(dropout_head0, sink_t=None, cu_doc=None, max_logits=False):    # ... and the optional ones behind them
            if max_logits:
                return (dropout_head0, sink_t, cu_doc, True)
            if cu_doc is not None:
                return (dropout_head0, sink_t, cu_doc)
            return (dropout_head0, sink_t) if sink_t is not None else ((dropout_head0,) if dropout_head0 else ())

        def func(q, k, v, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                 alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None,
                 attn_type: AttnType = AttnType.HIP, attn_processor=None, *, dropout_head0=0, sinks=None, cu_doclens=None,
                 bidirectional=None, block_mask=None, return_max_logits=False, block_select=None, return_block_mass=False):
            if return_block_mass_alone(return_block_mass, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional,
                                       block_mask, block_select, return_max_logits):
                return block_mass_call(serves, lambda probs: func(q, k, v, 0.0, softmax_scale, causal, deterministic=deterministic,
                                                                  return_attn_probs=probs, group=group, attn_type=attn_type,
                                                                  attn_processor=attn_processor),
                                       q, k, softmax_scale, causal, group, return_attn_probs)
            ml = max_logits_alone(return_max_logits, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional, block_mask,
                                  block_select=block_select)
            cu_doclens = block_mask_plan(block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional,
                                         block_select)
            cu_doclens = span_plan(q, group, cu_doclens, bidirectional)       # (the spans travel inside the plan from here on)
            D = q.shape[-1]
            if kernel_head_dim(D) != D:      # a head dim the kernels do not instantiate (e.g. 96): zero-padded copies
                res = func(*pad_head_dim(q, k, v), dropout_p, D ** -0.5 if softmax_scale is None else softmax_scale, causal,
                           window_size, softcap, alibi_slopes, deterministic, return_attn_probs, group, attn_type, attn_processor,
                           dropout_head0=dropout_head0, sinks=sinks, cu_doclens=cu_doclens, return_max_logits=ml)
                return (res[0][..., :D],) + tuple(res[1:]) if isinstance(res, tuple) else res[..., :D]
            if not needs_grad(q, k, v, *(() if sinks is None else (sinks,))):      # inference / forward-only benchmarks: no autograd node, no saved tensors (~25 us)
                done = run_forward(q, k, v, (), dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes, group,
                                   dict(zip(extra, last(attn_type, attn_processor))), dropout_head0, sinks, cu_doclens, ml)
                return result(done[4], done[5], (), return_attn_probs, done[7])
            return Func.apply(q, k, v, dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes, deterministic,
                              return_attn_probs, group, *last(attn_type, attn_processor), *head0_arg(dropout_head0, sinks, cu_doclens, ml))

        def kvpacked_func(q, kv, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                          alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None,
                          attn_type: AttnType = AttnType.HIP, *, dropout_head0=0, sinks=None, cu_doclens=None, bidirectional=None,
                          block_mask=None, return_max_logits=False, block_select=None, return_block_mass=False):
            if return_block_mass_alone(return_block_mass, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional,
                                       block_mask, block_select, return_max_logits):
                return block_mass_call(serves, lambda probs: kvpacked_func(q, kv, 0.0, softmax_scale, causal,
                                                                           deterministic=deterministic, return_attn_probs=probs,
                                                                           group=group, attn_type=attn_type),
                                       q, kv[:, :, 0], softmax_scale, causal, group, return_attn_probs)
            ml = max_logits_alone(return_max_logits, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional, block_mask,
                                  block_select=block_select)
            cu_doclens = block_mask_plan(block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional,
                                         block_select)
            cu_doclens = span_plan(q, group, cu_doclens, bidirectional)
            return Func.apply(q, kv[:, :, 0], kv[:, :, 1], dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes,
                              deterministic, return_attn_probs, group, *last(attn_type), *head0_arg(dropout_head0, sinks, cu_doclens, ml))

        def qkvpacked_func(qkv, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                           alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None,
                           attn_type: AttnType = AttnType.HIP, *, dropout_head0=0, sinks=None, cu_doclens=None, bidirectional=None,
                           block_mask=None, return_max_logits=False, block_select=None, return_block_mass=False):
            if return_block_mass_alone(return_block_mass, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional,
                                       block_mask, block_select, return_max_logits):
                return block_mass_call(serves, lambda probs: qkvpacked_func(qkv, 0.0, softmax_scale, causal,
                                                                            deterministic=deterministic, return_attn_probs=probs,
                                                                            group=group, attn_type=attn_type),
                                       qkv[:, :, 0], qkv[:, :, 1], softmax_scale, causal, group, return_attn_probs)
            ml = max_logits_alone(return_max_logits, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional, block_mask,
                                  block_select=block_select)
            cu_doclens = block_mask_plan(block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional,
                                         block_select)
            cu_doclens = span_plan(qkv[:, :, 0], group, cu_doclens, bidirectional)
            return Func.apply(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], dropout_p, softmax_scale, causal, window_size, softcap,
                              alibi_slopes, deterministic, return_attn_probs, group, *last(attn_type),
                              *head0_arg(dropout_head0, sinks, cu_doclens, ml))

    for fn, suffix in ((func, "_func"), (kvpacked_func, "_kvpacked_func"), (qkvpacked_func, "_qkvpacked_func")):
        fn.__name__ = fn.__qualname__ = stem + suffix
    return Func, func, kvpacked_func, qkvpacked_func
