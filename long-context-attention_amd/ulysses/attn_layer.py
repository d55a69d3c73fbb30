"""UlyssesAttention: same surface as yunchang/ulysses/attn_layer.py:15-126.

Pure head parallelism, i.e. LongContextAttention with ring degree 1: the sequence-sharded q, k, v are exchanged
into head shards, ONE local attention runs over the full sequence (the `fwd-bwd` stage of the kernel selector
= the HIP kernel with autograd), and the result is exchanged back.  The exchanges are SeqAllToAll4D
(comm/all_to_all.py: one pack pass, one RCCL all-to-all, the receive buffer consumed as a view).
"""
from typing import Any

import torch
import torch.distributed as dist
from torch import Tensor

from ..comm.all_to_all import SeqAllToAll4D, SeqAllToAll4DKV, layer_max_logits, local_options
from ..kernels import AttnType, select_flash_attn_impl
from ..kernels.features import block_mask_alone, block_select_alone, max_logits_alone, return_block_mass_alone


class UlyssesAttention(torch.nn.Module):
    """Constructor arguments as in the reference: sequence_process_group, scatter_idx (2 = heads), gather_idx
    (1 = sequence), use_sync (synchronise the device after each exchange), attn_type (any dense AttnType).
    forward takes the keyword-only `sinks`: one learned logit per head of the layer, (H,) (or per local head, (H / N,)), fp32 or
    the operands' type, cut to this rank's heads by slicing.  It is a parameter replicated over the group: each rank's gradient
    holds its own heads and zeros elsewhere, the SUM over the group is the gradient, and the layer does no all-reduce.
    `return_max_logits` (keyword only; beside window_size alone): the result is (out, max_logits), max_logits fp32 (H,) over the
    layer's heads without gradient: this rank's SHARE -- the largest visible pre-softmax logit of the heads it holds behind the
    exchange, -inf for the heads other ranks hold.  The MAX over the group is the value; the layer does no all-reduce.
    `return_block_mass` (keyword only; beside no other option): the result is (out, mass), mass fp32 (bs, H / N, nb, nb) without
    gradient: the block-pooled attention map (kernels/attention.py: block_attention_mass) of the heads this rank holds behind the
    exchange (comm/all_to_all.py: local_heads) over the whole sequence, from the call's own lse.  The layer gathers nothing."""

    def __init__(self, sequence_process_group: dist.ProcessGroup = None, scatter_idx: int = 2,
                 gather_idx: int = 1, use_sync: bool = False, attn_type: AttnType = AttnType.FA) -> None:
        super().__init__()
        self.spg, self.use_sync, self.attn_type = sequence_process_group, use_sync, attn_type
        self.scatter_idx, self.gather_idx = scatter_idx, gather_idx
        self.attn_fn = select_flash_attn_impl(attn_type, stage="fwd-bwd")

    def _to_heads(self, x: Tensor, kv: bool = False) -> Tensor:      # (bs, seq/N, heads, d) -> (bs, seq, heads/N, d)
        fn = SeqAllToAll4DKV if kv else SeqAllToAll4D            # (k, v: a KV head shared by several ranks is replicated)
        return fn.apply(self.spg, x, self.scatter_idx, self.gather_idx, self.use_sync, False)

    def _to_seq(self, x: Tensor) -> Tensor:        # (bs, seq, heads/N, d) -> (bs, seq/N, heads, d)
        return SeqAllToAll4D.apply(self.spg, x, self.gather_idx, self.scatter_idx, self.use_sync, False)

    def forward(self, query: Tensor, key: Tensor, value: Tensor, dropout_p=0.0, softmax_scale=None,
                causal=False, window_size=(-1, -1), softcap=0.0, alibi_slopes=None, deterministic=False,
                return_attn_probs=False, *args: Any, sinks=None, cu_doclens=None, bidirectional=None, block_mask=None,
                return_max_logits=False, block_select=None, return_block_mass=False) -> Tensor:
        # `return_block_mass`: judged alone and first (kernels/features.py: return_block_mass_alone)
        bm = return_block_mass_alone(return_block_mass, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional,
                                     block_mask, block_select, return_max_logits)
        # `return_max_logits`: judged alone (kernels/features.py: max_logits_alone)
        ml = max_logits_alone(return_max_logits, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional, block_mask,
                              block_select=block_select)
        # `block_select`: a BlockSelect or BlockSelectTopP: the block mask is selected behind the exchange, on this rank's heads over the whole
        # sequence (kernels/attention.py: select_blocks); judged alone, where block_mask is
        block_select_alone(block_select, block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional)
        # `block_mask`: a 128 x 128 block mask of the whole sequence (kernels/attention.py: hip_attn_forward), over the layer's
        # heads (cut to this rank's), the local heads or none; judged alone, before anything else
        block_mask_alone(block_mask, window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens, bidirectional)
        # `bidirectional`: spans of the whole sequence beside or without cu_doclens (kernels/attention.py: hip_attn_forward); an
        # empty list is the call without it.
        if bidirectional is not None and not isinstance(bidirectional, str) and len(bidirectional) == 0:
            bidirectional = None
        # what depends on the heads this rank holds behind the exchange (comm/all_to_all.py: local_options; cu_doclens is checked
        # against the whole sequence q then holds: kernels/features.py)
        head_kw, alibi_slopes = local_options(alibi_slopes, dropout_p, sinks, cu_doclens, query.shape[2],
                                              dist.get_world_size(self.spg), dist.get_rank(self.spg),
                                              (self.scatter_idx, self.gather_idx) == (2, 1), "scatter_idx=2, gather_idx=1",
                                              bidirectional=bidirectional, block_mask=block_mask, block_select=block_select,
                                              kv_heads=key.shape[2])
        q, k, v = (self._to_heads(t, kv) for t, kv in ((query, False), (key, True), (value, True)))
        options = dict(dropout_p=dropout_p, causal=causal, window_size=window_size, softcap=softcap,
                       alibi_slopes=alibi_slopes, deterministic=deterministic, return_attn_probs=return_attn_probs,
                       softmax_scale=q.shape[-1] ** -0.5 if softmax_scale is None else softmax_scale, **head_kw)
        attended = self.attn_fn(q, k, v, **options, **(dict(return_max_logits=True) if ml else {}),
                                **(dict(return_block_mass=True) if bm else {}))
        out = self._to_seq(attended[0] if isinstance(attended, tuple) else attended)
        if bm:
            return out, attended[-1]
        if not ml:
            return out
        return out, layer_max_logits(attended[-1], query.shape[2], dist.get_world_size(self.spg), dist.get_rank(self.spg))
