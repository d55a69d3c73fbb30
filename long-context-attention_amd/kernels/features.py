"""The optional features of one attention call -- window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens -- as ONE
record, and the ONE table of which of them the kernels serve together.  `bidirectional` (spans) is no seventh field: it goes
together with cu_doclens and RIDES INSIDE the parsed document plan (ring/doc_blocks.py: Spans), so the record keeps its six
fields and every positional construction its meaning; a `doc` that carries spans is named "bidirectional" in the refusals.
`block_mask` (a 128 x 128 block mask) is no field either: it goes with none of the seven and is judged in one place, before the
record is made (block_mask_alone).  `return_max_logits` (an extra RESULT, the largest visible logit of every head) likewise: it
goes with window_size alone (max_logits_alone).  `block_select` (a BlockSelect: the block mask is PRODUCED on the device,
kernels/attention.py: select_blocks) goes where block_mask goes, with nothing block_mask refuses and not with block_mask itself
(block_select_alone); it is a BlockSelect (a count) or a BlockSelectTopP (a cumulative softmax mass,
kernels/attention.py: select_blocks_top_p).  Pure argument logic: nothing here loads the library,
so the CPU orchestration tests import it as it is."""
from typing import NamedTuple

import torch

from .._C import HEAD_DIMS_QK_V, _window, alibi_value, antidiag_stride_value, block_select_top_p_value, block_select_value, dropout_value, sinks_value, softcap_value

# field of the record -> the flash-attn-style argument the messages name
ARGUMENT = dict(window="window_size", softcap="softcap", alibi="alibi_slopes", dropout="dropout_p", sinks="sinks", doc="cu_doclens")
# The combination table, a precedence list: the first feature that is on owns the call (its kernels run it), and beside it the
# listed ones are refused, in this order -- no kernel holds a second mask or score-level step.  A window goes with everything
# but the document mask.
REFUSES = (("doc", ("window", "softcap", "alibi", "dropout", "sinks")),
           ("sinks", ("softcap", "alibi", "dropout")),
           ("dropout", ("softcap", "alibi")),
           ("alibi", ("softcap",)),
           ("softcap", ()))
PACKED = ("softcap",)         # what the packed (variable-length) launches serve


BLOCK_MASK_SIZE = 128        # rows and keys of one block of `block_mask` (include/usp_hip.h: USP_BLOCK_MASK_SIZE)


def expand_block_mask(mask, block_size: int):
    """A block mask of `block_size`-square blocks (a multiple of BLOCK_MASK_SIZE) as the BLOCK_MASK_SIZE-square one the kernels
    take: every entry repeated block_size / BLOCK_MASK_SIZE times along the last two dimensions, on the mask's device."""
    if block_size <= 0 or block_size % BLOCK_MASK_SIZE:
        raise ValueError(f"block_size must be a positive multiple of {BLOCK_MASK_SIZE}, got {block_size}")
    n = block_size // BLOCK_MASK_SIZE
    return mask if n == 1 else mask.repeat_interleave(n, dim=-2).repeat_interleave(n, dim=-1)


def block_mask_alone(block_mask, window_size=None, softcap=None, alibi_slopes=None, dropout_p=None, sinks=None, cu_doclens=None,
                     bidirectional=None) -> bool:
    """Is `block_mask` on?  It is no field of the record: it is judged HERE, before Features.of and before any tensor is read,
    and goes with none of the other options -- the block-sparse kernels hold no second mask or score-level step.  None is
    exactly the call without the keyword."""
    if block_mask is None:
        return False
    given = (("window_size", _window(window_size)), ("softcap", softcap_value(softcap)), ("alibi_slopes", alibi_slopes),
             ("dropout_p", dropout_value(dropout_p)), ("sinks", sinks), ("cu_doclens", cu_doclens), ("bidirectional", bidirectional))
    for name, value in given:
        if value is not None:
            raise NotImplementedError(f"block_mask together with {name} is not supported by the HIP attention kernels")
    return True


class BlockSelect(NamedTuple):
    """`block_select=`: the block mask of the call is selected on the device from its own q and k -- top_k key blocks per
    (batch, query head, row block) by the score of the mean-pooled 128-blocks, the first `keep_first` key blocks and the last
    `keep_local` ones up to the row block's own always among them (kernels/attention.py: select_blocks).  Host integers."""
    top_k: int
    keep_first: int = 0
    keep_local: int = 1


class BlockSelectTopP(NamedTuple):
    """`block_select=` by cumulative mass: per (batch, query head, row block) the fewest key blocks whose softmax weight -- the
    softmax, over the visible blocks, of the scores of the mean-pooled 128-blocks -- reaches `top_p`; the first `keep_first` key
    blocks and the last `keep_local` ones up to the row block's own are always selected, and their mass counts.  `share_group`:
    the query heads of one KV head select together, on the mean of their weights, and get one mask row (NSA's rule)
    (kernels/attention.py: select_blocks_top_p).  Host values."""
    top_p: float
    keep_first: int = 0
    keep_local: int = 1
    share_group: bool = False


class BlockSelectAntidiag(NamedTuple):
    """`block_select=` by cumulative mass of ANTIDIAGONAL weights (XAttention's rule): the block weights come from every `stride`-th
    antidiagonal of the true score matrix (kernels/attention.py: antidiag_block_weights) where BlockSelectTopP pools means, so a
    few strong keys inside a block cannot hide; the cut is BlockSelectTopP's -- the fewest key blocks whose weight reaches
    `top_p`, the first `keep_first` and the last `keep_local` ones always among them (select_blocks_antidiag).  Host values;
    `stride` is 4, 8 or 16.  Ring degree 1 only."""
    top_p: float
    stride: int = 8
    keep_first: int = 0
    keep_local: int = 1


def block_select_antidiag_value(top_p, stride=8, keep_first=0, keep_local=1, causal=False):
    """The checked host values of a BlockSelectAntidiag: (top_p, stride, keep_first, keep_local); ValueError as
    _C.block_select_top_p_value, and for a stride that is no int of (4, 8, 16)."""
    top_p, keep_first, keep_local, _ = block_select_top_p_value(top_p, keep_first, keep_local, False, causal)
    return top_p, antidiag_stride_value(stride), keep_first, keep_local


def block_select_alone(block_select, block_mask=None, window_size=None, softcap=None, alibi_slopes=None, dropout_p=None, sinks=None,
                       cu_doclens=None, bidirectional=None) -> bool:
    """Is `block_select` on?  Judged HERE like block_mask (block_mask_alone), before any tensor is read: it goes with nothing
    block_mask goes without, and not with block_mask itself.  None is exactly the call without the keyword; anything but a
    BlockSelect, a BlockSelectTopP or a BlockSelectAntidiag raises ValueError, and so does a malformed one (_C.block_select_value,
    _C.block_select_top_p_value; keep_local under causal is judged where causal is known: select_blocks, select_blocks_top_p)."""
    if block_select is None:
        return False
    if not isinstance(block_select, (BlockSelect, BlockSelectTopP, BlockSelectAntidiag)):
        raise ValueError(f"block_select must be a BlockSelect(top_k, keep_first=0, keep_local=1) or a BlockSelectTopP(top_p, "
                         f"keep_first=0, keep_local=1, share_group=False) or a BlockSelectAntidiag(top_p, stride=8, keep_first=0, "
                         f"keep_local=1), got {type(block_select).__name__}")
    given = (("block_mask", block_mask), ("window_size", _window(window_size)), ("softcap", softcap_value(softcap)),
             ("alibi_slopes", alibi_slopes), ("dropout_p", dropout_value(dropout_p)), ("sinks", sinks), ("cu_doclens", cu_doclens),
             ("bidirectional", bidirectional))
    for name, value in given:
        if value is not None:
            raise NotImplementedError(f"block_select together with {name} is not supported by the HIP attention kernels")
    if isinstance(block_select, BlockSelectAntidiag):
        block_select_antidiag_value(*block_select)
    elif isinstance(block_select, BlockSelectTopP):
        block_select_top_p_value(*block_select)
    else:
        block_select_value(*block_select)
    return True


def max_logits_alone(return_max_logits, softcap=None, alibi_slopes=None, dropout_p=None, sinks=None, cu_doclens=None,
                     bidirectional=None, block_mask=None, block_select=None) -> bool:
    """Is `return_max_logits` on?  Like block_mask it is no field of the record: it is judged HERE, before Features.of and before
    any tensor is read.  It goes with window_size and nothing else -- the max-logit kernels hold no second mask or score-level
    step.  False / None is exactly the call without the keyword."""
    if not return_max_logits:
        return False
    given = (("softcap", softcap_value(softcap)), ("alibi_slopes", alibi_slopes), ("dropout_p", dropout_value(dropout_p)),
             ("sinks", sinks), ("cu_doclens", cu_doclens), ("bidirectional", bidirectional), ("block_mask", block_mask),
             ("block_select", block_select))
    for name, value in given:
        if value is not None:
            raise NotImplementedError(f"return_max_logits together with {name} is not supported by the HIP attention kernels")
    return True


def return_block_mass_alone(return_block_mass, window_size=None, softcap=None, alibi_slopes=None, dropout_p=None, sinks=None,
                            cu_doclens=None, bidirectional=None, block_mask=None, block_select=None, return_max_logits=False) -> bool:
    """Is `return_block_mass` on?  Like return_max_logits it is no field of the record: it is judged HERE, before Features.of and
    before any tensor is read.  The map is that of the plain softmax under the causal mask alone -- the kernel behind it
    (usp_block_attn_mass) holds no second mask and no score-level step -- so the keyword goes with none of the other options.
    (The stand-alone block_attention_mass takes whatever lse it is given: that is how a caller gets the map of a call with
    sinks.)  False / None is exactly the call without the keyword."""
    if not return_block_mass:
        return False
    given = (("window_size", _window(window_size)), ("softcap", softcap_value(softcap)), ("alibi_slopes", alibi_slopes),
             ("dropout_p", dropout_value(dropout_p)), ("sinks", sinks), ("cu_doclens", cu_doclens),
             ("bidirectional", bidirectional), ("block_mask", block_mask), ("block_select", block_select),
             ("return_max_logits", return_max_logits or None))
    for name, value in given:
        if value is not None:
            raise NotImplementedError(f"return_block_mass together with {name} is not supported by the HIP attention kernels")
    return True


def head_dim_256_alone(D: int, window_size=None, softcap=None, alibi_slopes=None, dropout_p=None, sinks=None, cu_doclens=None,
                        bidirectional=None, block_mask=None, block_select=None, return_max_logits=False, return_block_mass=False,
                        packed=False, key_index=None) -> bool:
    """Does a call of head dim `D` run at kernel head dim 256 (128 < D <= 256)?  That family (csrc/usp_flash_fwd_d256.hip,
    csrc/usp_flash_bwd_d256.hip) is the plain dense call -- causal or full, GQA, the rings' fused merge -- and nothing else: judged
    HERE like block_mask, before any tensor is read, it goes with none of the options, nor with a packed (variable-length) batch
    (`packed`).  A head dim above 256 is refused where it always was (kernels/attention.py: kernel_head_dim)."""
    if not 128 < D <= 256:
        return False
    given = (("window_size", _window(window_size)), ("softcap", softcap_value(softcap)), ("alibi_slopes", alibi_slopes),
             ("dropout_p", dropout_value(dropout_p)), ("sinks", sinks), ("cu_doclens", cu_doclens), ("bidirectional", bidirectional),
             ("block_mask", block_mask), ("block_select", block_select), ("return_max_logits", return_max_logits or None),
             ("return_block_mass", return_block_mass or None), ("a packed (variable-length) batch", packed or None),
             ("key_index", key_index))
    for name, value in given:
        if value is not None:
            raise NotImplementedError(f"head_dim {D} (kernel head dim 256) together with {name} is not supported by the HIP "
                                      f"attention kernels")
    return True


def head_dims_192_128_alone(D: int, Dv: int, window_size=None, softcap=None, alibi_slopes=None, dropout_p=None, sinks=None,
                            cu_doclens=None, bidirectional=None, block_mask=None, block_select=None, return_max_logits=False,
                            return_block_mass=False, packed=False, key_index=None) -> bool:
    """Does a call with q and k of head dim `D` and v of head dim `Dv` run on the (192, 128) family (csrc/usp_flash_fwd_qk192.hip,
    csrc/usp_flash_bwd_qk192.hip)?  False for equal head dims.  That family is the plain dense call -- causal or full, GQA, the
    rings' fused merge -- and nothing else: judged HERE like head_dim_256_alone, before any tensor is read, it goes with none of
    the options, nor with a packed (variable-length) batch (`packed`).  Any other unequal pair is refused, naming both dims: nothing
    is padded to (192, 128)."""
    if D == Dv:
        return False
    if (D, Dv) != HEAD_DIMS_QK_V:
        raise NotImplementedError(f"head_dim {D} of q and k with head_dim {Dv} of v is not supported by the HIP attention kernels: "
                                  f"unequal head dims are served for {HEAD_DIMS_QK_V} alone")
    given = (("window_size", _window(window_size)), ("softcap", softcap_value(softcap)), ("alibi_slopes", alibi_slopes),
             ("dropout_p", dropout_value(dropout_p)), ("sinks", sinks), ("cu_doclens", cu_doclens), ("bidirectional", bidirectional),
             ("block_mask", block_mask), ("block_select", block_select), ("return_max_logits", return_max_logits or None),
             ("return_block_mass", return_block_mass or None), ("a packed (variable-length) batch", packed or None),
             ("key_index", key_index))
    for name, value in given:
        if value is not None:
            raise NotImplementedError(f"head dims {HEAD_DIMS_QK_V} of q / k and v together with {name} are not supported by the HIP "
                                      f"attention kernels")
    return True


FP8_DTYPE = torch.float8_e4m3fn                  # OCP E4M3: the one 8-bit type the kernels take
_FP8_OTHERS = tuple(getattr(torch, n) for n in ("float8_e4m3fnuz", "float8_e5m2", "float8_e5m2fnuz", "float8_e8m0fnu") if hasattr(torch, n))
FP8_HEAD_DIM = 128
MX_SCALE_DTYPE = torch.float8_e8m0fnu             # OCP MX block scales: one power-of-two byte per 32 elements
MX_BLOCK = 32


def is_fp8(*tensors) -> bool:
    """Is any of the tensors (None allowed) of an 8-bit float type?"""
    return any(t is not None and t.dtype in (FP8_DTYPE,) + _FP8_OTHERS for t in tensors)


def mx_scales(q_descale, k_descale, v_descale) -> bool:
    """Are the descales of an e4m3 call MX block scales (csrc/usp_flash_fwd_mxfp8.hip)?  All three or none: fp8_alone has judged that."""
    return q_descale is not None and q_descale.dtype == MX_SCALE_DTYPE


def _mx_scales_alone(q, k, v, descales):
    """The MX form of the descales, from shapes, dtypes, devices and strides alone: all three in float8_e8m0fnu, q's and k's one byte per
    (token, head, 32-dim block), v's one per (32-key block, head, dim); last stride 1.  Mixed forms are refused by name."""
    mx = [name for name, t in descales if t is not None and t.dtype == MX_SCALE_DTYPE]
    if not mx:
        return
    for name, t in descales:
        if t is None or t.dtype != MX_SCALE_DTYPE:
            raise NotImplementedError(f"{name} is {'None' if t is None else t.dtype} beside {mx[0]} in torch.float8_e8m0fnu: MX block scales "
                                      f"go with all three of q_descale, k_descale and v_descale in torch.float8_e8m0fnu")
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    want = {"q_descale": (B, Sq, Hq, D // MX_BLOCK), "k_descale": (B, Sk, Hkv, D // MX_BLOCK),
            "v_descale": (B, (Sk + MX_BLOCK - 1) // MX_BLOCK, Hkv, D)}
    for name, t in descales:
        if tuple(t.shape) != want[name]:
            raise ValueError(f"{name} is {tuple(t.shape)}: the MX block scales of these operands are {want[name]}")
        if t.stride(-1) != 1:
            raise ValueError(f"{name} has a last stride of {t.stride(-1)}: MX block scales take a unit last stride")
        if t.device != q.device:
            raise ValueError(f"{name} is on {t.device}, the operands on {q.device}")


def fp8_forward_only(name: str, *tensors):
    """What every entry but hip_attn_forward answers to 8-bit operands."""
    if is_fp8(*tensors):
        raise NotImplementedError(f"{name} does not take float8 tensors: the fp8 path is forward-only and is reached through "
                                  f"hip_attn_forward (q, k, v in torch.float8_e4m3fn with q_descale / k_descale / v_descale)")


def fp8_alone(q, k, v, window_size=None, softcap=None, alibi_slopes=None, dropout_p=None, sinks=None, cu_doclens=None,
              bidirectional=None, block_mask=None, block_select=None, return_max_logits=False, return_block_mass=False,
              q_descale=None, k_descale=None, v_descale=None, key_index=None) -> bool:
    """Does a forward call run on the e4m3 family (csrc/usp_flash_fwd_fp8.hip)?  True when q, k and v are all torch.float8_e4m3fn.
    That family is the plain dense forward at head dim 128 -- causal or full, GQA, the fused merge -- and nothing else: judged HERE
    like head_dim_256_alone, before any tensor is read, it goes with none of the options and no other head dim (nothing is
    padded).  Mixed dtypes, the other 8-bit types, and descales beside 16-bit tensors are refused by name.  Descales in
    torch.float8_e8m0fnu are MX block scales (mx_scales: csrc/usp_flash_fwd_mxfp8.hip, the same rules): all three, of the block shapes."""
    dts = {"q": q.dtype, "k": k.dtype, "v": v.dtype}
    for name, dt in dts.items():
        if dt in _FP8_OTHERS:
            raise NotImplementedError(f"{name} is {dt}: the HIP attention kernels take torch.float8_e4m3fn (OCP E4M3) alone")
    n8 = sum(dt == FP8_DTYPE for dt in dts.values())
    if n8 == 0:
        for name, value in (("q_descale", q_descale), ("k_descale", k_descale), ("v_descale", v_descale)):
            if value is not None:
                raise NotImplementedError(f"{name} goes with torch.float8_e4m3fn q, k and v alone, got {dts['q']}")
        return False
    if n8 != 3:
        raise NotImplementedError(f"mixed dtypes {dts}: the fp8 forward takes q, k and v all in torch.float8_e4m3fn")
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.shape[-1] != FP8_HEAD_DIM:
            raise NotImplementedError(f"head_dim {t.shape[-1]} of {name} in float8_e4m3fn is not supported by the HIP attention "
                                      f"kernels: the fp8 forward serves head dim {FP8_HEAD_DIM} alone")
    given = (("window_size", _window(window_size)), ("softcap", softcap_value(softcap)), ("alibi_slopes", alibi_slopes),
             ("dropout_p", dropout_value(dropout_p)), ("sinks", sinks), ("cu_doclens", cu_doclens), ("bidirectional", bidirectional),
             ("block_mask", block_mask), ("block_select", block_select), ("return_max_logits", return_max_logits or None),
             ("return_block_mass", return_block_mass or None), ("key_index", key_index))
    for name, value in given:
        if value is not None:
            raise NotImplementedError(f"float8_e4m3fn q, k, v together with {name} are not supported by the HIP attention kernels")
    _mx_scales_alone(q, k, v, (("q_descale", q_descale), ("k_descale", k_descale), ("v_descale", v_descale)))
    return True


KEY_INDEX_HEAD_DIMS = (64, 128)


def key_index_alone(key_index, D: int, causal=True, window_size=None, softcap=None, alibi_slopes=None, dropout_p=None, sinks=None,
                    cu_doclens=None, bidirectional=None, block_mask=None, block_select=None, return_max_logits=False,
                    return_block_mass=False) -> bool:
    """Is `key_index` on (csrc/usp_flash_fwd_gather.hip; the semantics: include/usp_hip.h, USP_ATTN_KEY_INDEX)?  Like block_mask it is
    no field of the record: it is judged HERE, before Features.of and before any tensor is read.  It goes with window_size =
    (left, 0) -- the band below the diagonal -- and nothing else: the gathered-key kernel holds no other mask and no score-level
    step.  Causal calls of head dim 64 or 128 only (nothing is padded).  None is exactly the call without the keyword."""
    if key_index is None:
        return False
    win = _window(window_size)
    given = (("softcap", softcap_value(softcap)), ("alibi_slopes", alibi_slopes), ("dropout_p", dropout_value(dropout_p)),
             ("sinks", sinks), ("cu_doclens", cu_doclens), ("bidirectional", bidirectional), ("block_mask", block_mask),
             ("block_select", block_select), ("return_max_logits", return_max_logits or None),
             ("return_block_mass", return_block_mass or None),
             ("a window_size whose right bound is not 0", None if win is None or win[1] == 0 else win))
    for name, value in given:
        if value is not None:
            raise NotImplementedError(f"key_index together with {name} is not supported by the HIP attention kernels")
    if not causal:
        raise NotImplementedError("key_index together with causal=False is not supported by the HIP attention kernels: a row sees "
                                  "its listed keys up to the diagonal")
    if D not in KEY_INDEX_HEAD_DIMS:
        raise NotImplementedError(f"head_dim {D} together with key_index is not supported by the HIP attention kernels: the "
                                  f"gathered-key forward serves head dims {KEY_INDEX_HEAD_DIMS} alone")
    return True


def block_mask_self_attention(Sq: int, Sk: int, name: str = "block_mask"):
    """A block mask (given, or selected: `name`) covers one sequence against itself."""
    if Sq != Sk:
        raise NotImplementedError(f"{name} needs whole q and k of the same length (self-attention), got {Sq} and {Sk}: "
                                  f"for cross-attention use a dense call without the keyword")


class _SpanMark:
    """A `doc` value that stands for "a plan with spans is on" where only that matters (Features.check)."""
    spans = ()


SPAN_ON = _SpanMark()


def _argument(f, idx: int) -> str:
    """The argument the refusals name for field `idx` of the record `f`: a document plan with spans is `bidirectional`."""
    field = f._fields[idx]
    if field == "doc" and getattr(f[idx], "spans", None) is not None:
        return "bidirectional"
    return ARGUMENT[field]


class Features(NamedTuple):
    """The decoded options of one call; None = off.  window: (left, right); softcap: the cap, a float > 0; alibi: the slopes as
    the block calls take them; dropout: the drop probability in (0, 1); sinks: the logits as given (they may require grad);
    doc: the parsed document lists (ring/doc_blocks.py), with the bidirectional spans inside where they are on (Spans) -- or any
    marker where only "on" matters (SPAN_ON: on with spans)."""
    window: object = None
    softcap: object = None
    alibi: object = None
    dropout: object = None
    sinks: object = None
    doc: object = None

    @classmethod
    def of(cls, q, k, causal, window_size=None, softcap=None, alibi_slopes=None, dropout_p=None, sinks=None, cu_doclens=None,
           ring_degree: int = 1, bidirectional=None):
        """The checked record of a call with flash-attn-style arguments on q (B, Sq, Hq, D) and k, each rank holding 1 /
        ring_degree of the sequence.  ValueError: a malformed value (_C.softcap_value, dropout_value, alibi_value, sinks_value,
        doc_blocks.parse); NotImplementedError: a refused combination -- judged first, on what is given --, a document mask that is
        not causal self-attention.  A cu_doclens of one document is exactly the call without it: off -- after the checks.
        `bidirectional`: the spans of the whole sequence (doc_blocks.parse_plan), read FIRST: one that is off (None, empty, spans
        of length 1 only) is exactly the call without the keyword, whatever else is given; one that is on makes `doc` a plan with
        spans, refused beside the other five as "bidirectional together with ..." and where the call is not causal self-attention."""
        if bidirectional is not None:
            from ..ring import doc_blocks
            S_total = ring_degree * q.shape[1]
            plan = doc_blocks.parse_plan(cu_doclens, bidirectional, q.shape[0], S_total)
            if doc_blocks.spans_of(plan) is not None:
                f = cls(_window(window_size), softcap_value(softcap), alibi_slopes, dropout_value(dropout_p), sinks, plan).check()
                doc_blocks.refuse_not_causal_self(causal, S_total, ring_degree * k.shape[1], "bidirectional")
                return f
        f = cls(_window(window_size), softcap_value(softcap), alibi_slopes, dropout_value(dropout_p), sinks, cu_doclens)
        f.check()                                  # (on what is on and off: a refused pair is refused before a tensor or list is read)
        if cu_doclens is not None:
            from ..ring import doc_blocks
            docs = doc_blocks.parse(cu_doclens, q.shape[0], ring_degree * q.shape[1])
            doc_blocks.refuse_not_causal_self(causal, ring_degree * q.shape[1], ring_degree * k.shape[1],
                                              "cu_doclens" if doc_blocks.spans_of(docs) is None else "bidirectional")
            return f._replace(doc=None if docs is doc_blocks.SINGLE else docs)
        if alibi_slopes is not None:
            f = f._replace(alibi=alibi_value(alibi_slopes, q.shape[0], q.shape[2], q.device)[0])
        if sinks is not None:
            sinks_value(sinks, q.shape[2], q.device, q.dtype)
        return f

    def any(self) -> bool:                         # (by identity: `==` on a tensor field costs tens of microseconds)
        return not (self.window is None and self.softcap is None and self.alibi is None and self.dropout is None
                    and self.sinks is None and self.doc is None)

    def check(self):
        """Refuses what the table refuses; returns the record."""
        for owner, refused in _REFUSES_AT:
            if self[owner] is not None:
                for other in refused:
                    if self[other] is not None:
                        a, b = _argument(self, owner), _argument(self, other)
                        raise NotImplementedError(f"{a} together with {b} is not supported by the HIP attention kernels")
                break
        return self

    def refuse_packed(self):
        """Refuses what the packed (variable-length) launches do not serve."""
        for field, name in ARGUMENT.items():
            if field != "window" and field not in PACKED and getattr(self, field) is not None:
                if field == "doc" and getattr(self.doc, "spans", None) is not None:
                    name = "bidirectional"
                raise NotImplementedError(f"{name} is not supported on packed (variable-length) batches")


# REFUSES by position in the record (check runs on every call, the plain one too)
_REFUSES_AT = tuple((Features._fields.index(owner), tuple(Features._fields.index(other) for other in refused))
                    for owner, refused in REFUSES)
