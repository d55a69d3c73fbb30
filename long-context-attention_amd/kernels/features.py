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

from .._C import _window, alibi_value, block_select_top_p_value, block_select_value, dropout_value, sinks_value, softcap_value

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


def block_select_alone(block_select, block_mask=None, window_size=None, softcap=None, alibi_slopes=None, dropout_p=None, sinks=None,
                       cu_doclens=None, bidirectional=None) -> bool:
    """Is `block_select` on?  Judged HERE like block_mask (block_mask_alone), before any tensor is read: it goes with nothing
    block_mask goes without, and not with block_mask itself.  None is exactly the call without the keyword; anything but a
    BlockSelect or a BlockSelectTopP raises ValueError, and so does a malformed one (_C.block_select_value,
    _C.block_select_top_p_value; keep_local under causal is judged where causal is known: select_blocks, select_blocks_top_p)."""
    if block_select is None:
        return False
    if not isinstance(block_select, (BlockSelect, BlockSelectTopP)):
        raise ValueError(f"block_select must be a BlockSelect(top_k, keep_first=0, keep_local=1) or a BlockSelectTopP(top_p, "
                         f"keep_first=0, keep_local=1, share_group=False), got {type(block_select).__name__}")
    given = (("block_mask", block_mask), ("window_size", _window(window_size)), ("softcap", softcap_value(softcap)),
             ("alibi_slopes", alibi_slopes), ("dropout_p", dropout_value(dropout_p)), ("sinks", sinks), ("cu_doclens", cu_doclens),
             ("bidirectional", bidirectional))
    for name, value in given:
        if value is not None:
            raise NotImplementedError(f"block_select together with {name} is not supported by the HIP attention kernels")
    if isinstance(block_select, BlockSelectTopP):
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
