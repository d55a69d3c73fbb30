"""Ulysses head <-> sequence all-to-all: same surface as yunchang/comm/all_to_all.py:15-134.

MI355X-first differences (results identical):
  * one HBM pass per exchange instead of two: the reference copies before AND after
    `all_to_all_single` (all_to_all.py:45-49 and :62-65 / :76-84 and :98-100).  Inside this package the
    receive buffer of the head-scatter exchange is used as a strided (B,S,H/P,D) VIEW of its natural
    (S,B,H/P,D) layout -- the attention kernels take strides -- and the send buffer of the
    sequence-scatter exchange is that same layout, which the kernels write directly (the PUBLIC
    functions and autograd Functions return contiguous tensors like the reference's unless asked not to);
  * the remaining pack / unpack is one `usp_copy_rows` launch (16-byte lanes, rows of H/P*D);
  * P == 1 moves no bytes at all (the reference still makes two copies).
The collective itself is `torch.distributed.all_to_all_single` == RCCL over xGMI on ROCm.
"""
from typing import Any, Tuple

import torch
import torch.distributed as dist
from torch import Tensor

from .._C import dropout_value
from ..kernels.attention import get_block_backend
from . import relay_exchange


def seq_major_empty(B, S, H, D, dtype, device):
    """A (B,S,H,D) view over an (S,B,H,D)-contiguous buffer: the layout both all-to-all directions
    exchange without a copy."""
    return torch.empty((S, B, H, D), dtype=dtype, device=device).transpose(0, 1)


def is_seq_major(x: Tensor) -> bool:
    B, S, H, D = x.shape
    return x.transpose(0, 1).is_contiguous()


def _copy_rows(dst: Tensor, src: Tensor, row_elems: int, sizes, dst_strides, src_strides):
    """dst/src: base tensors; strides in elements.  Device tensors -> usp_copy_rows; host tensors
    (gloo orchestration tests) -> as_strided copy."""
    es = src.element_size()
    if src.is_cuda:
        get_block_backend().copy_rows(dst, src, row_elems * es, list(sizes),
                                      [s * es for s in dst_strides], [s * es for s in src_strides])
    else:
        # host tensors (gloo orchestration tests): hold the copy to what usp_copy_rows takes (include/usp_hip.h: row
        # bytes, every stride and both pointers multiples of 16), so a layout the device path would refuse fails here too
        assert (row_elems * es) % 16 == 0 and all((st * es) % 16 == 0 for st in list(dst_strides) + list(src_strides)) \
            and (dst.storage_offset() * es) % 16 == 0 and (src.storage_offset() * es) % 16 == 0, \
            f"usp_copy_rows needs 16-byte rows / strides / pointers: row {row_elems * es} B, strides {dst_strides} {src_strides}"
        d = torch.as_strided(dst, list(sizes) + [row_elems], list(dst_strides) + [1],
                             dst.storage_offset())
        s = torch.as_strided(src, list(sizes) + [row_elems], list(src_strides) + [1],
                             src.storage_offset())
        d.copy_(s)


def _sum_rows(dst: Tensor, src: Tensor, row_elems: int, r: int, term_stride: int, sizes, dst_strides, src_strides):
    """dst rows = the sum of r src rows `term_stride` elements apart (fp32, ascending term order, rounded once).  Device
    tensors -> usp_sum_rows; host tensors (gloo orchestration tests) -> the same sum over as_strided views."""
    es = src.element_size()
    if src.is_cuda:
        get_block_backend().sum_rows(dst, src, row_elems * es, r, term_stride * es, list(sizes),
                                     [s * es for s in dst_strides], [s * es for s in src_strides])
    else:
        # host tensors: the constraints of usp_sum_rows (include/usp_hip.h), as _copy_rows holds copies to usp_copy_rows'
        assert (row_elems * es) % 16 == 0 and (term_stride * es) % 16 == 0 \
            and all((st * es) % 16 == 0 for st in list(dst_strides) + list(src_strides)) \
            and (dst.storage_offset() * es) % 16 == 0 and (src.storage_offset() * es) % 16 == 0, \
            f"usp_sum_rows needs 16-byte rows / strides / pointers: row {row_elems * es} B, strides {dst_strides} {src_strides}"
        d = torch.as_strided(dst, list(sizes) + [row_elems], list(dst_strides) + [1], dst.storage_offset())
        acc = torch.zeros(d.shape, dtype=torch.float32)
        for t in range(r):
            acc = acc + torch.as_strided(src, list(sizes) + [row_elems], list(src_strides) + [1],
                                         src.storage_offset() + t * term_stride).float()
        d.copy_(acc)


def _exchange(send: Tensor, group, use_sync: bool) -> Tensor:
    if relay_exchange.applicable(send, group):       # a pair's exchange striped over the idle mesh links (opt-in)
        recv = relay_exchange.exchange_relayed(send, group)
        if use_sync and send.is_cuda:
            torch.cuda.synchronize()
        return recv
    recv = torch.empty_like(send)
    dist.all_to_all_single(recv, send, group=group)
    if use_sync and send.is_cuda:
        torch.cuda.synchronize()
    return recv


def pack_heads(x: Tensor, P: int) -> Tensor:
    """(B, S/P, H, D) -> send buffer (P, S/P, B, H/P, D): chunk p goes to ulysses rank p."""
    B, Sl, H, D = x.shape
    assert H % P == 0, f"head count {H} not divisible by ulysses degree {P}"
    hp = H // P
    if x.stride(3) != 1 or x.stride(2) != D:
        x = x.contiguous()
    send = torch.empty((P, Sl, B, hp, D), dtype=x.dtype, device=x.device)
    _copy_rows(send, x, hp * D, (P, Sl, B), (Sl * B * hp * D, B * hp * D, hp * D),
               (hp * D, x.stride(1), x.stride(0)))
    return send


def local_heads(H: int, P: int, rank: int) -> slice:
    """THE rank -> query-head map of the head-scatter exchange: pack_heads sends chunk p = heads [p H/P, (p+1) H/P) to
    ulysses rank p, so that is what rank `rank` holds behind it."""
    assert H % P == 0, f"head count {H} not divisible by ulysses degree {P}"
    hp = H // P
    return slice(rank * hp, (rank + 1) * hp)


def local_alibi_slopes(alibi_slopes, H: int, P: int, rank: int):
    """flash-attn's alibi_slopes for the heads ulysses rank `rank` holds behind the head-scatter exchange of an H-head layer.
    A tensor over the layer's H heads, (H,) or (B, H), is cut to them (local_heads); one over the local H / P heads -- what
    the reference requires of its caller (it forwards the tensor untouched to a block of H / P heads) -- is taken as it is;
    any other length raises ValueError.  None stays None."""
    if alibi_slopes is None or P == 1:
        return alibi_slopes
    n = alibi_slopes.shape[-1] if alibi_slopes.dim() in (1, 2) else -1
    if n == H:
        return alibi_slopes[..., local_heads(H, P, rank)].contiguous()
    if H % P == 0 and n == H // P:
        return alibi_slopes
    raise ValueError(f"alibi_slopes must cover the layer's {H} heads or the {H // max(P, 1)} heads of one ulysses rank "
                     f"(shape (H,) or (B, H)), got {tuple(alibi_slopes.shape)}")


def local_sinks(sinks, H: int, P: int, rank: int):
    """The sink logits (one per query head) of the heads ulysses rank `rank` holds behind the head-scatter exchange of an H-head
    layer.  A tensor over the layer's H heads is cut to them by SLICING (local_heads), so autograd scatters the rank's gradient
    back into a (H,) gradient that is zero elsewhere; one over the local H / P heads is taken as it is; any other shape raises
    ValueError.  None stays None."""
    if sinks is None or P == 1:
        return sinks
    n = sinks.shape[0] if sinks.dim() == 1 else -1
    if n == H:
        return sinks[local_heads(H, P, rank)]
    if H % P == 0 and n == H // P:
        return sinks
    raise ValueError(f"sinks must cover the layer's {H} heads or the {H // max(P, 1)} heads of one ulysses rank (shape (H,)), "
                     f"got {tuple(sinks.shape)}")


def layer_max_logits(max_logits: Tensor, H: int, P: int, rank: int) -> Tensor:
    """The share of ulysses rank `rank` in the max logits of an H-head layer (return_max_logits): fp32 (H,) holding the maxima of
    the heads the rank holds behind the head-scatter exchange (local_heads) and -inf for the heads other ranks hold, so that the
    MAX over the sequence-parallel group is the value -- the replication contract of the sinks' gradient with max in the place of
    sum.  The layers do no all-reduce.  No host read."""
    if P == 1:
        return max_logits
    out = torch.full((H,), float("-inf"), dtype=torch.float32, device=max_logits.device)
    out[local_heads(H, P, rank)] = max_logits
    return out


def local_block_mask(block_mask, H: int, P: int, rank: int):
    """The block mask of the heads ulysses rank `rank` holds behind the head-scatter exchange of an H-head layer.  One with a
    head dimension over the layer's H heads, (H, nb, nb) or (B, H, nb, nb), is cut to them (local_heads: a view, no copy); one
    over the local H / P heads, or without a head dimension, is taken as it is; any other head count raises ValueError.  None
    stays None.  Never read on the host."""
    if block_mask is None or P == 1 or block_mask.dim() < 3:
        return block_mask
    n = block_mask.shape[-3]
    if n == H:
        return block_mask[..., local_heads(H, P, rank), :, :]
    if H % P == 0 and n == H // P:
        return block_mask
    raise ValueError(f"block_mask must cover the layer's {H} heads or the {H // max(P, 1)} heads of one ulysses rank, "
                     f"got {tuple(block_mask.shape)}")


def local_options(alibi_slopes, dropout_p, sinks, cu_doclens, H: int, P: int, rank: int, head_scatter: bool, how: str,
                  bidirectional=None, block_mask=None, block_select=None, kv_heads=None):
    """What a layer of H heads hands its attention function for the options that depend on WHICH heads ulysses rank `rank` of P
    holds behind the exchange: (keyword dict, local slopes).
      alibi_slopes  cut to the rank's heads (local_alibi_slopes);
      dropout_p     `dropout_head0`: the mask is keyed by the layer's GLOBAL query head (include/usp_hip.h:
                    usp_flash_fwd_dropout), KV-replicated grids included -- the counter holds the query head;
      sinks         cut to the rank's heads by slicing (local_sinks), so autograd scatters the gradient back.  The sinks are a
                    parameter replicated over the sequence-parallel group: each rank's gradient is its share (its rows of the
                    ring, its heads under Ulysses, zeros elsewhere), the SUM over the group is the gradient, and the layers do
                    no all-reduce;
      cu_doclens    as given: the list describes the WHOLE sequence and is the same on every rank; behind the exchange a rank
                    holds whole rows of some heads, so the attention function plans its arrays alone (ring/doc_blocks.py).
      bidirectional as given, likewise (a layer that has parsed it already hands the plan over as `cu_doclens`: the spans ride
                    inside, ring/doc_blocks.py: Spans).
      block_select  as given: the selection has no cross-head term, so behind the exchange the attention function selects for the
                    heads the rank holds over the whole sequence it then holds (kernels/attention.py: select_blocks).  A
                    BlockSelectTopP with share_group adds the weights of the query heads of one KV head: served where every
                    rank holds whole groups (P <= `kv_heads`, the layer's KV heads), refused (NotImplementedError) where the
                    KV heads are replicated over ranks (kv_heads < P) and a group's heads live on several of them.
    Each of them needs an exchange that scatters heads and gathers the sequence (`head_scatter`; `how`: that, in the layer's
    words): NotImplementedError otherwise."""
    p = dropout_value(dropout_p)
    if not head_scatter:
        doc_name = "cu_doclens" if getattr(cu_doclens, "spans", None) is None else "bidirectional"
        for name, value in (("alibi_slopes", alibi_slopes), ("dropout_p != 0", p), ("sinks", sinks), (doc_name, cu_doclens),
                            ("bidirectional", bidirectional), ("block_mask", block_mask), ("block_select", block_select)):
            if value is not None:
                raise NotImplementedError(f"{name} needs the head-scatter exchange ({how})")
    if getattr(block_select, "share_group", False) and P > 1 and kv_heads is not None and kv_heads % P:
        raise NotImplementedError(f"block_select with share_group=True needs every ulysses rank to hold whole KV groups, got "
                                  f"{kv_heads} KV heads over ulysses degree {P} (a group's query heads live on several ranks): "
                                  f"use share_group=False or a ulysses degree that divides the KV heads")
    kw = {}
    if p is not None and P > 1:
        kw["dropout_head0"] = local_heads(H, P, rank).start
    if sinks is not None:
        kw["sinks"] = local_sinks(sinks, H, P, rank)
    if cu_doclens is not None:
        kw["cu_doclens"] = cu_doclens
    if bidirectional is not None:
        kw["bidirectional"] = bidirectional
    if block_mask is not None:                     # cut to the rank's heads (local_block_mask)
        kw["block_mask"] = local_block_mask(block_mask, H, P, rank)
    if block_select is not None:
        kw["block_select"] = block_select
    return kw, local_alibi_slopes(alibi_slopes, H, P, rank)


def pack_head_group(x5: Tensor, send: Tensor = None, h0: int = 0) -> Tensor:
    """x5: a (B, S/P, P, h, D) VIEW (any strides on the first three dims, (h, D) contiguous) selecting
    h heads per destination rank -> heads [h0, h0+h) of the send buffer (P, S/P, B, Ht, D) (allocated with
    Ht = h when not given).  Used by the head-group pipeline; q, k and v of a group share ONE send buffer
    (Ht = hq + 2 hkv per rank and group), i.e. one collective instead of three."""
    B, Sl, P, h, D = x5.shape
    assert x5.stride(4) == 1 and x5.stride(3) == D
    if send is None:
        send = torch.empty((P, Sl, B, h, D), dtype=x5.dtype, device=x5.device)
    Ht = send.shape[3]
    assert send.shape == (P, Sl, B, Ht, D) and send.is_contiguous() and h0 + h <= Ht
    base = x5.as_strided((1,), (1,), x5.storage_offset())          # element pointer of the view
    dst = send.as_strided((1,), (1,), send.storage_offset() + h0 * D)
    _copy_rows(dst, base, h * D, (P, Sl, B), (Sl * B * Ht * D, B * Ht * D, Ht * D),
               (x5.stride(2), x5.stride(1), x5.stride(0)))
    return send


def unpack_head_group(recv: Tensor, dst5: Tensor, h0: int = 0) -> None:
    """heads [h0, h0+h) of the receive buffer (P, S/P, B, Ht, D) [chunk p = head group of rank p] -> dst5, a
    (B, S/P, P, h, D) VIEW into the full (B, S/P, H, D) result."""
    P, Sl, B, Ht, D = recv.shape
    h = dst5.shape[3]
    assert dst5.stride(4) == 1 and dst5.stride(3) == D and h0 + h <= Ht
    base = dst5.as_strided((1,), (1,), dst5.storage_offset())
    src = recv.as_strided((1,), (1,), recv.storage_offset() + h0 * D)
    _copy_rows(base, src, h * D, (P, Sl, B), (dst5.stride(2), dst5.stride(1), dst5.stride(0)),
               (Sl * B * Ht * D, B * Ht * D, Ht * D))


def pack_seq_into(send: Tensor, h0: int, x: Tensor) -> None:
    """(B, S, h, D) -> heads [h0, h0+h) of the sequence-scatter send buffer (P, S/P, B, Ht, D)."""
    P, Sl, B, Ht, D = send.shape
    h = x.shape[2]
    assert x.shape == (B, P * Sl, h, D) and h0 + h <= Ht and send.is_contiguous()
    if x.stride(3) != 1 or x.stride(2) != D:
        x = x.contiguous()
    dst = send.as_strided((1,), (1,), send.storage_offset() + h0 * D)
    base = x.as_strided((1,), (1,), x.storage_offset())
    _copy_rows(dst, base, h * D, (P * Sl, B), (B * Ht * D, Ht * D), (x.stride(1), x.stride(0)))


def pack_seq_rows(x: Tensor, P: int, lo: int, hi: int) -> Tensor:
    """Rows [lo, hi) of EVERY destination's chunk of (B, S, h, D) -> a send buffer (P, hi - lo, B, h, D) of its own: one piece
    of a row-chunked sequence-scatter exchange (hybrid/async_attn_layer.py: tails).  Destination p owns rows [p S/P, (p+1) S/P)."""
    B, S, h, D = x.shape
    assert S % P == 0 and 0 <= lo < hi <= S // P
    Sl, n = S // P, hi - lo
    if x.stride(3) != 1 or x.stride(2) != D:
        x = x.contiguous()
    send = torch.empty((P, n, B, h, D), dtype=x.dtype, device=x.device)
    base = x.as_strided((1,), (1,), x.storage_offset() + lo * x.stride(1))
    _copy_rows(send, base, h * D, (P, n, B), (n * B * h * D, B * h * D, h * D), (Sl * x.stride(1), x.stride(1), x.stride(0)))
    return send


def view_seq(recv: Tensor) -> Tensor:
    """receive buffer (P, S/P, B, H/P, D) -> (B, S, H/P, D) strided view (no copy)."""
    P, Sl, B, hp, D = recv.shape
    return recv.view(P * Sl, B, hp, D).transpose(0, 1)


def pack_seq(x: Tensor, P: int) -> Tensor:
    """(B, S, H/P, D) -> send buffer (P, S/P, B, H/P, D); free when x is already seq-major."""
    B, S, hp, D = x.shape
    assert S % P == 0, f"sequence {S} not divisible by ulysses degree {P}"
    if is_seq_major(x):
        send = x.transpose(0, 1)                       # already (S,B,hp,D) contiguous: no copy
    else:
        if x.stride(3) != 1 or x.stride(2) != D:
            x = x.contiguous()
        send = torch.empty((S, B, hp, D), dtype=x.dtype, device=x.device)
        _copy_rows(send, x, hp * D, (S, B), (B * hp * D, hp * D), (x.stride(1), x.stride(0)))
    return send.view(P, S // P, B, hp, D)


def unpack_heads(recv: Tensor) -> Tensor:
    """receive buffer (P, S/P, B, H/P, D) [chunk p = head group p] -> (B, S/P, H, D) contiguous."""
    P, Sl, B, hp, D = recv.shape
    H = hp * P
    out = torch.empty((B, Sl, H, D), dtype=recv.dtype, device=recv.device)
    _copy_rows(out, recv, hp * D, (P, Sl, B), (hp * D, H * D, Sl * H * D),
               (Sl * B * hp * D, B * hp * D, hp * D))
    return out


def heads_to_seq(x: Tensor, group, use_sync: bool = False, contiguous: bool = False) -> Tensor:
    """scatter heads / gather sequence: (B, S/P, H, D) -> (B, S, H/P, D)  (all_to_all.py:36-67)."""
    P = dist.get_world_size(group)
    if P == 1:
        return x
    out = view_seq(_exchange(pack_heads(x, P), group, use_sync))
    return out.contiguous() if contiguous else out


def seq_to_heads(x: Tensor, group, use_sync: bool = False) -> Tensor:
    """scatter sequence / gather heads: (B, S, H/P, D) -> (B, S/P, H, D)  (all_to_all.py:69-102)."""
    P = dist.get_world_size(group)
    if P == 1:
        return x
    return unpack_heads(_exchange(pack_seq(x, P), group, use_sync))


def all_to_all_4D(input: torch.Tensor, scatter_idx: int = 2, gather_idx: int = 1, group=None,
                  use_sync: bool = False) -> torch.Tensor:
    """Public function with the reference's semantics (contiguous result)."""
    assert input.dim() == 4, f"input must be 4D tensor, got {input.dim()} and shape {input.shape}"
    if scatter_idx == 2 and gather_idx == 1:
        return heads_to_seq(input, group, use_sync, contiguous=True)
    if scatter_idx == 1 and gather_idx == 2:
        return seq_to_heads(input, group, use_sync)
    raise RuntimeError("scatter_idx must be 1 or 2 and gather_idx must be 1 or 2")


class SeqAllToAll4D(torch.autograd.Function):
    """all_to_all.py:105-134: forward = the exchange, backward = the inverse exchange.  Like the reference the
    result is CONTIGUOUS.  The layers of this package pass `contiguous=False` (a sixth positional argument the
    reference does not have): the head-scatter result is then the strided (B,S,H/P,D) VIEW of the receive buffer,
    which the attention kernels consume directly (they take strides) -- one HBM pass less per exchange."""

    @staticmethod
    def forward(ctx: Any, group, input: Tensor, scatter_idx: int, gather_idx: int,
                use_sync: bool = False, contiguous: bool = True) -> Tensor:
        ctx.group = group
        ctx.scatter_idx = scatter_idx
        ctx.gather_idx = gather_idx
        ctx.use_sync = use_sync
        ctx.contiguous = contiguous
        if scatter_idx == 2 and gather_idx == 1:
            return heads_to_seq(input, group, use_sync, contiguous=contiguous)
        if scatter_idx == 1 and gather_idx == 2:
            return seq_to_heads(input, group, use_sync)
        raise RuntimeError("scatter_idx must be 1 or 2 and gather_idx must be 1 or 2")

    @staticmethod
    def backward(ctx: Any, *grad_output: Tensor) -> Tuple[None, Tensor, None, None, None, None]:
        return (None,
                SeqAllToAll4D.apply(ctx.group, grad_output[0], ctx.gather_idx, ctx.scatter_idx,
                                    ctx.use_sync, ctx.contiguous),
                None, None, None, None)


# --------------------------------------------------------------------------------------------------
# KV heads shared by several Ulysses ranks: Hkv < P, P % Hkv == 0 (MQA, or 4 KV heads at ulysses degree 8)
# --------------------------------------------------------------------------------------------------
def kv_replicas(Hkv: int, P: int) -> int:
    """r, the number of Ulysses ranks that share one KV head after the head-scatter exchange -- THE rank -> KV-head map
    of this package (every pack, unpack and layer below asks here):
        Hkv % P == 0           r = 1: rank p owns KV heads [p Hkv/P, (p+1) Hkv/P), the exchange as ever;
        Hkv < P, P % Hkv == 0  r = P / Hkv: rank p gets KV head p // r, a REPLICA, beside its query heads
                               [p Hq/P, (p+1) Hq/P) (they all use that head when Hq % P == 0: Hq/P divides G = Hq/Hkv).
                               Forward: every rank sends its rows of head h to ranks h r .. h r + r - 1.  Backward: a
                               rank's dK/dV is a partial sum over its own query heads; each sequence owner sums the r
                               partials of a head in fp32, in ascending Ulysses rank order, and rounds once;
        otherwise              0: not served."""
    if Hkv % P == 0:
        return 1
    return P // Hkv if P % Hkv == 0 else 0


def pack_kv_replicated(send: Tensor, h0: int, x: Tensor, r: int) -> None:
    """(B, S/P, Hkv, D) with Hkv r == P -> head h0 of the send buffer (P, S/P, B, Ht, D): chunk p (destination rank p)
    gets KV head p // r (kv_replicas).  ONE usp_copy_rows launch whose source stride over the r replicas is zero."""
    P, Sl, B, Ht, D = send.shape
    Hkv = x.shape[2]
    assert r > 1 and Hkv * r == P and x.shape == (B, Sl, Hkv, D) and send.is_contiguous() and h0 < Ht
    if x.stride(3) != 1:
        x = x.contiguous()
    dst = send.as_strided((1,), (1,), send.storage_offset() + h0 * D)
    base = x.as_strided((1,), (1,), x.storage_offset())
    chunk = Sl * B * Ht * D
    _copy_rows(dst, base, D, (Hkv, r, Sl, B), (r * chunk, chunk, B * Ht * D, Ht * D),
               (x.stride(2), 0, x.stride(1), x.stride(0)))


def unpack_kv_sum(recv: Tensor, dst: Tensor, h0: int, r: int) -> None:
    """The inverse for gradients: head h0 of the receive buffer (P, S/P, B, Ht, D) [chunk p = rank p's partial of KV head
    p // r over this rank's rows] -> dst (B, S/P, Hkv, D), head h = the sum of chunks h r .. h r + r - 1 (usp_sum_rows)."""
    P, Sl, B, Ht, D = recv.shape
    Hkv = dst.shape[2]
    assert r > 1 and Hkv * r == P and dst.shape == (B, Sl, Hkv, D) and dst.stride(3) == 1 and h0 < Ht
    src = recv.as_strided((1,), (1,), recv.storage_offset() + h0 * D)
    base = dst.as_strided((1,), (1,), dst.storage_offset())
    chunk = Sl * B * Ht * D
    _sum_rows(base, src, D, r, chunk, (Hkv, Sl, B), (dst.stride(2), dst.stride(1), dst.stride(0)),
              (r * chunk, B * Ht * D, Ht * D))


def kv_heads_to_seq(x: Tensor, group, use_sync: bool = False, contiguous: bool = False) -> Tensor:
    """heads_to_seq for K or V: (B, S/P, Hkv, D) -> (B, S, Hkv/P, D), or (B, S, 1, D) = KV head p // r on rank p when the
    head is shared (kv_replicas)."""
    P = dist.get_world_size(group)
    r = kv_replicas(x.shape[2], P) if P > 1 else 1
    if r <= 1:
        return heads_to_seq(x, group, use_sync, contiguous)
    B, Sl, _, D = x.shape
    send = torch.empty((P, Sl, B, 1, D), dtype=x.dtype, device=x.device)
    pack_kv_replicated(send, 0, x, r)
    out = view_seq(_exchange(send, group, use_sync))
    return out.contiguous() if contiguous else out


def kv_seq_to_heads(x: Tensor, group, Hkv: int, use_sync: bool = False) -> Tensor:
    """The gradient direction of kv_heads_to_seq: (B, S, h, D) -> (B, S/P, Hkv, D); with a shared head the r partials of
    every KV head are summed (unpack_kv_sum)."""
    P = dist.get_world_size(group)
    r = kv_replicas(Hkv, P) if P > 1 else 1
    if r <= 1:
        return seq_to_heads(x, group, use_sync)
    B, S, _, D = x.shape
    recv = _exchange(pack_seq(x, P), group, use_sync)
    out = torch.empty((B, S // P, Hkv, D), dtype=x.dtype, device=x.device)
    unpack_kv_sum(recv, out, 0, r)
    return out


class SeqAllToAll4DKV(torch.autograd.Function):
    """SeqAllToAll4D for K and V (same arguments): where the KV heads divide among the ranks (kv_replicas = 1) -- and for
    any other direction or head count -- it IS SeqAllToAll4D (same collectives, launches and errors); where r ranks share a
    head, the forward sends every rank its replica and the backward sums the r gradient partials of each head."""

    @staticmethod
    def forward(ctx: Any, group, input: Tensor, scatter_idx: int, gather_idx: int,
                use_sync: bool = False, contiguous: bool = True) -> Tensor:
        P = dist.get_world_size(group)
        r = kv_replicas(input.shape[2], P) if P > 1 and (scatter_idx, gather_idx) == (2, 1) else 1
        ctx.kv_heads = input.shape[2] if r > 1 else 0
        if r <= 1:
            return SeqAllToAll4D.forward(ctx, group, input, scatter_idx, gather_idx, use_sync, contiguous)
        ctx.group, ctx.use_sync = group, use_sync
        return kv_heads_to_seq(input, group, use_sync, contiguous)

    @staticmethod
    def backward(ctx: Any, *grad_output: Tensor) -> Tuple[None, Tensor, None, None, None, None]:
        if not ctx.kv_heads:
            return SeqAllToAll4D.backward(ctx, *grad_output)
        return (None, kv_seq_to_heads(grad_output[0], ctx.group, ctx.kv_heads, ctx.use_sync), None, None, None, None)


# --------------------------------------------------------------------------------------------------
# packed qkv: (bs, seq, 3, heads, dim)   (yunchang/comm/all_to_all.py:137-259)
# --------------------------------------------------------------------------------------------------
def pack_heads_5d(x: Tensor, P: int) -> Tensor:
    """(B, S/P, T, H, D) -> send buffer (P, S/P, B, T, H/P, D)."""
    B, Sl, T, H, D = x.shape
    assert H % P == 0, f"head count {H} not divisible by ulysses degree {P}"
    hp = H // P
    if x.stride(4) != 1 or x.stride(3) != D:
        x = x.contiguous()
    send = torch.empty((P, Sl, B, T, hp, D), dtype=x.dtype, device=x.device)
    _copy_rows(send, x, hp * D, (P, Sl, B, T),
               (Sl * B * T * hp * D, B * T * hp * D, T * hp * D, hp * D),
               (hp * D, x.stride(1), x.stride(0), x.stride(2)))
    return send


def view_seq_5d(recv: Tensor) -> Tensor:
    P, Sl, B, T, hp, D = recv.shape
    return recv.view(P * Sl, B, T, hp, D).transpose(0, 1)


def pack_seq_5d(x: Tensor, P: int) -> Tensor:
    B, S, T, hp, D = x.shape
    assert S % P == 0, f"sequence {S} not divisible by ulysses degree {P}"
    if x.transpose(0, 1).is_contiguous():
        send = x.transpose(0, 1)
    else:
        if not x[0, 0].is_contiguous():
            x = x.contiguous()
        send = torch.empty((S, B, T, hp, D), dtype=x.dtype, device=x.device)
        _copy_rows(send, x, T * hp * D, (S, B), (B * T * hp * D, T * hp * D), (x.stride(1), x.stride(0)))
    return send.view(P, S // P, B, T, hp, D)


def unpack_heads_5d(recv: Tensor) -> Tensor:
    P, Sl, B, T, hp, D = recv.shape
    H = hp * P
    out = torch.empty((B, Sl, T, H, D), dtype=recv.dtype, device=recv.device)
    _copy_rows(out, recv, hp * D, (P, Sl, B, T), (hp * D, T * H * D, Sl * T * H * D, H * D),
               (Sl * B * T * hp * D, B * T * hp * D, T * hp * D, hp * D))
    return out


def heads_to_seq_5d(x: Tensor, group, use_sync: bool = False, contiguous: bool = False) -> Tensor:
    """scatter heads / gather sequence: (B, S/P, T, H, D) -> (B, S, T, H/P, D) -- ONE exchange for
    q, k and v (all_to_all.py:160-192)."""
    P = dist.get_world_size(group)
    if P == 1:
        return x
    out = view_seq_5d(_exchange(pack_heads_5d(x, P), group, use_sync))
    return out.contiguous() if contiguous else out


def seq_to_heads_5d(x: Tensor, group, use_sync: bool = False) -> Tensor:
    """scatter sequence / gather heads: (B, S, T, H/P, D) -> (B, S/P, T, H, D) (all_to_all.py:193-233)."""
    P = dist.get_world_size(group)
    if P == 1:
        return x
    return unpack_heads_5d(_exchange(pack_seq_5d(x, P), group, use_sync))


def all_to_all_5D(input: torch.Tensor, scatter_idx: int = 3, gather_idx: int = 1, group=None,
                  use_sync: bool = False) -> torch.Tensor:
    assert input.dim() == 5, f"input must be 5D tensor, got {input.dim()} and shape {input.shape}"
    if scatter_idx == 3 and gather_idx == 1:
        assert input.shape[2] == 3
        return heads_to_seq_5d(input, group, use_sync, contiguous=True)
    if scatter_idx == 1 and gather_idx == 3:
        return seq_to_heads_5d(input, group, use_sync)
    raise RuntimeError("scatter_idx must be 1 or 3 and gather_idx must be 1 or 3")


class SeqAllToAll5D(torch.autograd.Function):
    """all_to_all.py:236-259; `contiguous` as in SeqAllToAll4D."""

    @staticmethod
    def forward(ctx: Any, group, input: Tensor, scatter_idx: int = 3, gather_idx: int = 1,
                use_sync: bool = False, contiguous: bool = True) -> Tensor:
        ctx.group = group
        ctx.scatter_idx = scatter_idx
        ctx.gather_idx = gather_idx
        ctx.use_sync = use_sync
        ctx.contiguous = contiguous
        if scatter_idx == 3 and gather_idx == 1:
            return heads_to_seq_5d(input, group, use_sync, contiguous=contiguous)
        if scatter_idx == 1 and gather_idx == 3:
            return seq_to_heads_5d(input, group, use_sync)
        raise RuntimeError("scatter_idx must be 1 or 3 and gather_idx must be 1 or 3")

    @staticmethod
    def backward(ctx: Any, *grad_output: Tensor) -> Tuple[None, Tensor, None, None, None, None]:
        return (None,
                SeqAllToAll5D.apply(ctx.group, grad_output[0], ctx.gather_idx, ctx.scatter_idx,
                                    ctx.use_sync, ctx.contiguous),
                None, None, None, None)
