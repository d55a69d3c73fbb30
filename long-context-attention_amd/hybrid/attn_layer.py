"""LongContextAttention: same surface as yunchang/hybrid/attn_layer.py:14-161.

forward = Ulysses head all-to-all of q, k, v (attn_layer.py:111-119) -> ring attention over the
ring group (:132-147) -> all-to-all of the output back to sequence sharding (:156-158).

MI355X-first: q, k and v travel in ONE packed head all-to-all (GQA-capable), and the exchanges are pipelined over
head groups on a side HIP stream behind the attention kernels instead of running exposed in front of and behind
them (LongContextAttention._packed_exchange); results are identical.
"""
import os
from typing import Any

import torch
import torch.distributed as dist
from torch import Tensor

from .._C import dropout_value, softcap_value
from ..comm.all_to_all import SeqAllToAll4D, SeqAllToAll4DKV, SeqAllToAll5D, kv_replicas, layer_max_logits, local_options
from ..globals import PROCESS_GROUP
from ..kernels import AttnType
from ..kernels.attention import kernel_head_dim, pad_head_dim, window_of
from ..kernels.features import block_mask_alone, block_select_alone, max_logits_alone, return_block_mass_alone
from ..ring import doc_blocks
from ..ring.front_end import _check_hot_path_args
from .async_attn_layer import _AsyncUSPFunc, _MAX_GROUPS, _RING_FWD_BWD, pipeline_mode
from .utils import RING_IMPL_DICT, RING_IMPL_QKVPACKED_DICT


def _first(result):
    """Ring functions return `out` or `(out, lse, None)`; the layers only hand `out` on."""
    return result[0] if isinstance(result, tuple) else result


class _USPLayer(torch.nn.Module):
    """What both layers share: the 2-D process grid of set_seq_parallel_pg and the two exchanges."""

    def __init__(self, scatter_idx: int, gather_idx: int, use_sync: bool, attn_type: AttnType) -> None:
        super().__init__()
        self.ring_pg, self.ulysses_pg = PROCESS_GROUP.RING_PG, PROCESS_GROUP.ULYSSES_PG
        assert (
            self.ulysses_pg is not None or self.ring_pg is not None
        ), f"use set_seq_parallel_pg() first. Now ulysses pg {self.ulysses_pg} and ring pg {self.ring_pg}"
        self.scatter_idx, self.gather_idx = scatter_idx, gather_idx
        self.use_sync, self.attn_type = use_sync, attn_type
        self._ulysses_size = self._ring_size = None

    @property
    def ulysses_size(self) -> int:
        """Ulysses degree; the grid is fixed once the groups exist, so torch.distributed is asked once (on the
        first forward -- the constructor, like the reference's, only checks that a group is set)."""
        if self._ulysses_size is None:
            self._ulysses_size = dist.get_world_size(self.ulysses_pg)
        return self._ulysses_size

    @property
    def ring_size(self) -> int:
        if self._ring_size is None:
            self._ring_size = dist.get_world_size(self.ring_pg) if self.ring_pg is not None else 1
        return self._ring_size

    def _head_options(self, alibi_slopes, dropout_p, sinks, cu_doclens, heads: int, scatter_idx: int, block_mask=None,
                      block_select=None, kv_heads=None):
        """(the ring function's keywords dropout_head0 / sinks / cu_doclens, the slopes) for the heads this Ulysses rank holds
        behind the exchange (comm/all_to_all.py: local_options); with nothing to exchange any layout serves."""
        P = self.ulysses_size
        return local_options(alibi_slopes, dropout_p, sinks, cu_doclens, heads, P, dist.get_rank(self.ulysses_pg) if P > 1 else 0,
                             P == 1 or (scatter_idx, self.gather_idx) == (2, 1), "heads scattered, sequence gathered",
                             block_mask=block_mask, block_select=block_select, kv_heads=kv_heads)

    def _docs(self, cu_doclens, batch: int, local_len: int, bidirectional=None):
        """`cu_doclens` checked against the WHOLE sequence (ring/doc_blocks.py: parse; a rank holds local_len of its
        ulysses_size x ring_size x local_len positions): the parsed lists, or None when it is off or names the single document
        [0, S_total] -- which is exactly the call without it, the same exchange and the same launches.  `bidirectional`: the spans
        of the whole sequence (doc_blocks.parse_plan); where they are on, the plan that comes back carries them, and it travels on
        as `cu_doclens`; where they are off (None, empty, length 1 only) the result is that of `cu_doclens` alone."""
        if cu_doclens is None and bidirectional is None:
            return None
        docs = doc_blocks.parse_plan(cu_doclens, bidirectional, batch, self.ulysses_size * self.ring_size * local_len)
        return None if docs is doc_blocks.SINGLE else docs

    def _max_logits(self, result, heads: int):
        """This rank's share of the layer's max logits from the ring function's result (its last element: the ring's share, the
        rows of this ring rank, over the heads this Ulysses rank holds): fp32 (heads,), -inf for the heads other Ulysses ranks
        hold (comm/all_to_all.py: layer_max_logits).  The MAX over the sequence-parallel group is the value; no all-reduce here."""
        P = self.ulysses_size
        return layer_max_logits(result[-1], heads, P, dist.get_rank(self.ulysses_pg) if P > 1 else 0)

    def _ring_options(self, dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes, deterministic,
                      return_attn_probs):
        return dict(dropout_p=dropout_p, softmax_scale=softmax_scale, causal=causal, window_size=window_size,
                    softcap=softcap, alibi_slopes=alibi_slopes, deterministic=deterministic,
                    return_attn_probs=return_attn_probs, group=self.ring_pg, attn_type=self.attn_type)


class LongContextAttention(_USPLayer):
    """Unified sequence parallel attention (ulysses x ring), arguments as in the reference:
        scatter_idx / gather_idx (int): dims of the all-to-all (2 = heads, 1 = sequence)
        ring_impl_type (str): key of RING_IMPL_DICT ("basic" | "zigzag" | "strip")
        use_pack_qkv (bool): q, k and v travel in ONE head all-to-all instead of three.  This layer ALWAYS
            packs (GQA-capable buffer (P, S/P, B, hq + 2 hkv, D), hybrid/async_attn_layer.py:_qkv_to_seq) --
            the flag is accepted and changes nothing; results are identical either way.  (The reference's
            packed branch is dead code: `.continous()` typo at attn_layer.py:88, and it cannot express GQA.)
            USP_PACK_QKV=0 restores the reference's three-exchange structure (an A/B switch for multi-GPU
            measurements).
        use_sync (bool): synchronise the device after each all-to-all (three blocking exchanges, as the
            reference)
        attn_type (AttnType): any dense type; all are served by the gfx950 kernel
    Beside packing, the exchange is PIPELINED over head groups on a side HIP stream behind the attention
    kernels whenever there is more than one group to pipeline (hybrid/async_attn_layer.py:pipeline_mode:
    USP_PIPELINE_ULYSSES=0 disables it, =1 enables it also beside a ring, USP_SAFE_COMM=1 keeps ONE communicator
    in flight at any time).
    """

    def __init__(self, scatter_idx: int = 2, gather_idx: int = 1, ring_impl_type: str = "basic",
                 use_pack_qkv: bool = False, use_sync: bool = False,
                 attn_type: AttnType = AttnType.FA, attn_processor: torch.nn.Module = None) -> None:
        super().__init__(scatter_idx, gather_idx, use_sync, attn_type)
        self.use_pack_qkv = use_pack_qkv
        self.attn_processor = attn_processor
        self.ring_attn_fn = RING_IMPL_DICT[ring_impl_type]
        self.ring_impl_type = ring_impl_type

    def _packed_exchange(self, query: Tensor, key: Tensor):
        """None: exchange q, k, v separately (the reference's structure); otherwise the cap on the number of
        head groups of the packed exchange (1 = one packed exchange in front of the attention and one behind
        it; more = pipelined over head groups on the side stream, hybrid/async_attn_layer.py -- identical
        results).  See `pipeline_mode` for when the exchange is pipelined."""
        if self.ulysses_size == 1:
            return None
        if os.environ.get("USP_PACK_QKV", "1") == "0" or self.use_sync or self.attn_processor is not None:
            return None
        if (self.scatter_idx, self.gather_idx) != (2, 1) or self.ring_impl_type not in _RING_FWD_BWD:
            return None
        P = self.ulysses_size
        if query.shape[2] % P or not kv_replicas(key.shape[2], P):     # (KV heads shared by P / Hkv ranks: served)
            return None
        return _MAX_GROUPS if pipeline_mode(self.ring_size) else 1

    def forward(self, query: Tensor, key: Tensor, value: Tensor, dropout_p=0.0, softmax_scale=None,
                causal=False, window_size=(-1, -1), softcap=0.0, alibi_slopes=None,
                deterministic=False, return_attn_probs=False, *args: Any, sinks=None, cu_doclens=None,
                bidirectional=None, block_mask=None, return_max_logits=False, block_select=None,
                return_block_mass=False) -> Tensor:
        """query (bs, seq_len/N, head_cnt, head_size); key/value (bs, seq_len/N, kv_head_cnt,
        head_size) -> context (bs, seq_len/N, head_cnt, head_size).  `sinks` (keyword only): one learned logit per head of the
        layer, (head_cnt,) fp32 or the operands' type (comm/all_to_all.py: local_options: the gradient contract).  `cu_doclens` (keyword
        only): the cumulative document lengths of the WHOLE sequence, host data, the same on every rank (ring/doc_blocks.py):
        global row i sees global key j iff start(i) <= j <= i.  Needs causal=True; served with the basic ring at any ring
        degree, with the zigzag and stripe rings at ring degree 1.  `bidirectional` (keyword only): half-open spans [(s, e), ...]
        of global positions of the WHOLE sequence, host data, the same on every rank, or "documents" (ring/doc_blocks.py:
        parse_plan): inside a span every row sees the whole span; with or without cu_doclens, served where it is.  None, an empty
        list or spans of length 1 only: exactly the call without it -- the same exchange and the same launches.
        `block_mask` (keyword only): a torch.bool DEVICE tensor of 128 x 128 blocks over the WHOLE sequence, the same on every
        rank, (nb, nb), (head_cnt, nb, nb) or (bs, head_cnt, nb, nb) (or over the local heads): global row i sees global key j iff
        block_mask[b, h, i // 128, j // 128] and (not causal or j <= i).  Never read on the host; not together with any other
        option.  Served with the basic ring at any ring degree (a local length that is a multiple of 128), with the zigzag and
        stripe rings at ring degree 1, through three exchanges.  None: exactly the call without it.
        `return_max_logits` (keyword only; beside window_size alone): the result is (context, max_logits), max_logits fp32
        (head_cnt,) without gradient: this rank's SHARE of the largest visible pre-softmax logit of every head -- its rows of the
        ring, the heads it holds under Ulysses, -inf for the heads other ranks hold.  The MAX over the sequence-parallel group is
        the value (QK-clip takes it); the layer does no all-reduce and reads nothing on the host.  Through three exchanges.
        `block_select` (keyword only): a BlockSelect(top_k, keep_first=0, keep_local=1) or a BlockSelectTopP(top_p, keep_first=0,
        keep_local=1, share_group=False; kernels/attention.py: select_blocks_top_p): the block mask is SELECTED on the device,
        behind the head exchange, from the q and k of the whole sequence (kernels/attention.py: select_blocks) -- the call with
        block_mask=select_blocks(q, k, ...) of the gathered sequence and the layer's heads.  Served where block_mask is (on a ring
        of degree > 1 each rank pools its slices and the pooled keys are all-gathered: ring/front_end.py: select_block_rows); not
        together with block_mask or anything block_mask refuses.  None: exactly the call without it.
        `return_block_mass` (keyword only; beside no other option): the result is (context, mass), mass fp32 without gradient: this
        rank's SHARE of the block-pooled attention map of the whole sequence (kernels/attention.py: block_attention_mass) -- the
        heads it holds behind the exchange (comm/all_to_all.py: local_heads) and its ring shard's n row blocks against all nb key
        blocks, (bs, head_cnt / ulysses degree, n, nb) (ring/front_end.py: ring_block_attention_mass: K alone makes a second
        rotation behind the forward, from the exchanged k and the ring's lse).  The layer gathers nothing and reads nothing on
        the host.  Served with the basic ring at any ring degree (a local length behind the exchange that is a multiple of
        128), with the zigzag and stripe rings at ring degree 1, through three exchanges."""
        bmass = return_block_mass_alone(return_block_mass, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens,
                                        bidirectional, block_mask, block_select, return_max_logits)
        ml = max_logits_alone(return_max_logits, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional, block_mask,
                              block_select=block_select)
        block_select_alone(block_select, block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional)
        block_mask_alone(block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional)
        D = query.shape[-1]
        if kernel_head_dim(D) != D:      # a head dim the kernels do not instantiate (e.g. 96): zero-padded copies
            out = self.forward(*pad_head_dim(query, key, value), dropout_p, D ** -0.5 if softmax_scale is None else softmax_scale,
                               causal, window_size, softcap, alibi_slopes, deterministic, return_attn_probs, *args, sinks=sinks,
                               cu_doclens=cu_doclens, bidirectional=bidirectional, block_mask=block_mask, return_max_logits=ml,
                               block_select=block_select, return_block_mass=bmass)
            return (out[0][..., :D], out[1]) if ml or bmass else out[..., :D]
        cu_doclens = self._docs(cu_doclens, query.shape[0], query.shape[1], bidirectional)     # (the single document: None from here on)
        ng_cap = self._packed_exchange(query, key)
        if ng_cap is not None and (block_mask is not None or block_select is not None or cu_doclens is not None or window_of(window_size) is not None or alibi_slopes is not None
                                   or dropout_value(dropout_p) is not None or sinks is not None or ml or bmass):
            # Any of them: the reference's structure (three exchanges), and the ring function serves it (ring/front_end.py: _place).
            # The pipeline issues blocks in row pieces and head groups: under a document mask each piece would need its own
            # arrays; a sliding window is served by the basic ring function at ring degree 1 and, with USP_RING_WINDOW=global,
            # beyond (ring/ring_flash_attn.py); ALiBi would need a slice of the slopes and a shift per piece and group; dropout
            # their place in the mask; and the pieces open a row range more than once (ring/block_pieces.py), where a sink
            # must count once.
            ng_cap = None
        if ng_cap is not None:
            _check_hot_path_args(dropout_p, window_size, softcap)
            return _AsyncUSPFunc.apply(query, key, value, softmax_scale, causal, self.ulysses_pg, self.ring_pg,
                                       self.ring_impl_type, ng_cap, softcap_value(softcap))
        head_kw, alibi_slopes = self._head_options(alibi_slopes, dropout_p, sinks, cu_doclens, query.shape[2], self.scatter_idx,
                                                   block_mask, block_select, key.shape[2])
        options = self._ring_options(dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes, deterministic,
                                     return_attn_probs)
        options.update(head_kw)
        if ml:
            options["return_max_logits"] = True
        if bmass:
            options["return_block_mass"] = True
        if self.ulysses_size == 1:      # nothing to exchange (the reference still makes 8 layout copies here)
            res = self.ring_attn_fn(query, key, value, attn_processor=self.attn_processor, **options)
            if bmass:
                return _first(res), res[-1]
            return (_first(res), self._max_logits(res, query.shape[2])) if ml else _first(res)
        # sequence shards -> head shards: (bs, seq_len/N, heads, d) -> (bs, seq_len, heads/N, d); k and v through the KV
        # form (a KV head shared by several ranks travels to each of them, and their gradients are summed)
        q, k, v = (fn.apply(self.ulysses_pg, t, self.scatter_idx, self.gather_idx, self.use_sync, False)
                   for fn, t in ((SeqAllToAll4D, query), (SeqAllToAll4DKV, key), (SeqAllToAll4DKV, value)))
        res = self.ring_attn_fn(q, k, v, attn_processor=self.attn_processor, **options)
        # ... and back: (bs, seq_len, heads/N, d) -> (bs, seq_len/N, heads, d)
        context = SeqAllToAll4D.apply(self.ulysses_pg, _first(res), self.gather_idx, self.scatter_idx, self.use_sync, False)
        if bmass:                       # (the ring function's share: this rank's heads, its ring shard's row blocks)
            return context, res[-1]
        return (context, self._max_logits(res, query.shape[2])) if ml else context


class LongContextAttentionQKVPacked(_USPLayer):
    """Same surface as yunchang/hybrid/attn_layer.py:164-259: packed
    qkv (bs, seq_len/N, 3, head_cnt, head_size) -> ONE head all-to-all (instead of three) -> ring
    attention on the packed views -> all-to-all of the output back.  Equal head counts only
    (a packed tensor cannot express GQA, README.md:193)."""

    def __init__(self, scatter_idx: int = 3, gather_idx: int = 1, ring_impl_type: str = "basic",
                 use_sync: bool = False, attn_type: AttnType = AttnType.FA) -> None:
        super().__init__(scatter_idx, gather_idx, use_sync, attn_type)
        self.ring_attn_fn = RING_IMPL_QKVPACKED_DICT[ring_impl_type]

    def forward(self, qkv, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1),
                softcap=0.0, alibi_slopes=None, deterministic=False, return_attn_probs=False,
                *args: Any, sinks=None, cu_doclens=None, bidirectional=None, block_mask=None, return_max_logits=False,
                block_select=None, return_block_mass=False) -> Tensor:
        """`return_max_logits` (keyword only): (out, max_logits) as LongContextAttention.forward returns it.  `block_select`
        (keyword only): as LongContextAttention.forward takes it.  `return_block_mass` (keyword only): (out, mass) as
        LongContextAttention.forward returns it."""
        bmass = return_block_mass_alone(return_block_mass, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens,
                                        bidirectional, block_mask, block_select, return_max_logits)
        ml = max_logits_alone(return_max_logits, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional, block_mask,
                              block_select=block_select)
        block_select_alone(block_select, block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional)
        block_mask_alone(block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional)
        D = qkv.shape[-1]
        if kernel_head_dim(D) != D:
            out = self.forward(pad_head_dim(qkv)[0], dropout_p, D ** -0.5 if softmax_scale is None else softmax_scale, causal,
                               window_size, softcap, alibi_slopes, deterministic, return_attn_probs, *args, sinks=sinks,
                               cu_doclens=cu_doclens, bidirectional=bidirectional, block_mask=block_mask, return_max_logits=ml,
                               block_select=block_select, return_block_mass=bmass)
            return (out[0][..., :D], out[1]) if ml or bmass else out[..., :D]
        exchange = self.ulysses_size > 1
        cu_doclens = self._docs(cu_doclens, qkv.shape[0], qkv.shape[1], bidirectional)
        head0, alibi_slopes = self._head_options(alibi_slopes, dropout_p, sinks, cu_doclens, qkv.shape[3], self.scatter_idx - 1,
                                                 block_mask, block_select, qkv.shape[3])
        if exchange:         # scatter 3 (heads), gather 1 (sequence)
            qkv = SeqAllToAll5D.apply(self.ulysses_pg, qkv, self.scatter_idx, self.gather_idx, self.use_sync, False)
        heads = qkv.shape[3] * (self.ulysses_size if exchange else 1)          # (of the layer: qkv holds this rank's by now)
        res = self.ring_attn_fn(qkv, **self._ring_options(dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes,
                                                          deterministic, return_attn_probs), **head0,
                                **(dict(return_max_logits=True) if ml else {}), **(dict(return_block_mass=True) if bmass else {}))
        out = _first(res)
        if exchange:         # (bs, seq_len, head_cnt/N, head_size) -> (bs, seq_len/N, head_cnt, head_size)
            out = SeqAllToAll4D.apply(self.ulysses_pg, out, self.gather_idx, self.scatter_idx - 1,
                                      self.use_sync, False)
        if bmass:
            return out, res[-1]
        return (out, self._max_logits(res, heads)) if ml else out
