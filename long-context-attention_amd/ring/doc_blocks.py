"""Document mask (`cu_doclens`): the host-side planner.

A sequence that packs several documents keeps every row from attending across a document boundary: with start(i) the first
position of the document that holds global position i, global row i sees global key j iff start(i) <= j <= i.  `cu_doclens` is
the list of cumulative document lengths of the WHOLE sequence, before any sharding: host integers [0, e1, ..., S_total], strictly
increasing, as a Python sequence or a CPU integer tensor; one list shared by the batch, or a sequence of B such lists.

Everything here is host arithmetic (numpy): no torch.distributed, no device value is ever read.  For one launch -- the global
positions of its rows and of its keys, two contiguous ranges -- the planner gives the two int32 arrays the kernels take
(include/usp_hip.h: usp_flash_fwd_doc / usp_flash_bwd_doc), in the launch's own coordinates, both non-decreasing:
    row_lo[i] = clamp(start(row0 + i) - key0, 0, n_keys)     the first key row i sees; n_keys: none
    key_hi[j] = #{i : row_lo[i] <= j}                        one past the last row that sees key j under this bound
or says that nothing is visible, in which case the launch is dropped on the host.  The causal bound is not folded in: the
diagonal block of a ring runs the causal kernel, the blocks below it the full one.  All arrays of a call are built first and go
to the device in ONE copy (DocCall.upload).

Bidirectional spans (`bidirectional`): a list of half-open ranges [(s0, e0), ...] of global positions, sorted and pairwise
disjoint, each inside one document; inside a span every row sees the whole span.  With hi(i) = e of the span that holds i, or
i + 1 where no span does, global row i sees global key j iff start(i) <= j < hi(i).  parse_plan() folds the spans into the parsed
lists (Spans: the lists plus, per list, its spans -- one object travels where `cu_doclens` travels), and for a plan with spans
the planner gives FOUR arrays per launch (include/usp_hip.h: usp_flash_fwd_span / usp_flash_bwd_span), all non-decreasing:
    row_lo[i] = clamp(start(row0 + i) - key0, 0, n_keys)     row_hi[i] = clamp(hi(row0 + i) - key0, 0, n_keys)
    key_lo[j] = #{i : row_hi[i] <= j}                        key_hi[j] = #{i : row_lo[i] <= j}
with the causal diagonal folded into row_hi: such launches are never causal.  A `cu_doclens`-only part of the same call is
served through the same arrays (hi(i) = i + 1 is just another monotone bound).
Why both bounds are non-decreasing in i: start(i) is constant on a document and jumps to a larger value at the next one.  For
hi: take i < i'.  If no span holds i, hi(i) = i + 1 <= i' < hi(i').  If the span [s, e) holds i and also i', hi is e for both.  If
it holds i and not i', then i' >= e (i' > i >= s and i' is outside), so hi(i') >= i' + 1 > e = hi(i) -- the spans being disjoint
and sorted is what makes "outside and to the right" mean "at or past e".  Clamping keeps the order.
"""
import numpy as np
import torch

SINGLE = "single"        # parse(): the list is one document -- exactly the call without it


class Docs(tuple):
    """What parse() returns for a list it has checked: a tuple of one list (shared by the batch) or B lists, each a tuple of
    ints.  parse() hands it back as it is, so a layer may parse once and pass the result down."""


class Spans(Docs):
    """A checked plan WITH bidirectional spans: the lists as Docs holds them, and `.spans`, one tuple of (s, e) pairs per
    list (spans of length 1 dropped: they change nothing).  A plan without `cu_doclens` holds the one document (0, S_total)."""

    def __new__(cls, docs, spans):
        self = super().__new__(cls, docs)
        self.spans = tuple(spans)
        assert len(self.spans) == len(self)
        return self


def spans_of(docs):
    """The per-list spans of a parsed plan, or None for one without any."""
    return getattr(docs, "spans", None)


def _one_list(cu, S_total):
    if isinstance(cu, torch.Tensor):
        if cu.device.type != "cpu":
            raise ValueError("cu_doclens must be host data (a Python sequence or a CPU integer tensor), got a tensor on "
                             f"{cu.device}: the planner reads it without a device sync")
        if cu.dtype.is_floating_point or cu.dtype == torch.bool or cu.dim() != 1:
            raise ValueError(f"cu_doclens must be a 1-D integer tensor, got {cu.dtype} of shape {tuple(cu.shape)}")
        cu = cu.tolist()
    cu = [int(x) for x in cu]
    if len(cu) < 2 or cu[0] != 0:
        raise ValueError(f"cu_doclens must start at 0 and hold at least one document, got {cu[:4]}...")
    if any(b <= a for a, b in zip(cu, cu[1:])):
        raise ValueError("cu_doclens must be strictly increasing (no empty document)")
    if cu[-1] != S_total:
        raise ValueError(f"cu_doclens must end at the whole sequence length {S_total}, got {cu[-1]}")
    return tuple(cu)


def parse(cu_doclens, B: int, S_total: int):
    """`cu_doclens` -> None (off), SINGLE (every list is the one document [0, S_total]: the call without the keyword), or a
    tuple of one list (shared by the batch) or B lists, each a tuple of ints.  ValueError: a device tensor, a list that does
    not start at 0, is not strictly increasing or does not end at S_total, B lists for another B."""
    if cu_doclens is None or cu_doclens is SINGLE or isinstance(cu_doclens, Docs):
        if isinstance(cu_doclens, Docs) and (len(cu_doclens) not in (1, B) or any(c[-1] != S_total for c in cu_doclens)):
            raise ValueError(f"cu_doclens was checked for another batch or sequence length than ({B}, {S_total})")
        return cu_doclens
    if isinstance(cu_doclens, torch.Tensor):
        if cu_doclens.device.type != "cpu":
            raise ValueError(f"cu_doclens must be host data (a Python sequence or a CPU integer tensor), got a tensor on "
                             f"{cu_doclens.device}: the planner reads it without a device sync")
        nested = cu_doclens.dim() == 2
        lists = list(cu_doclens) if nested else [cu_doclens]
    else:
        cu_doclens = list(cu_doclens)
        nested = len(cu_doclens) > 0 and isinstance(cu_doclens[0], (list, tuple, torch.Tensor, np.ndarray))
        lists = cu_doclens if nested else [cu_doclens]
    if nested and len(lists) != B:
        raise ValueError(f"cu_doclens holds {len(lists)} lists for a batch of {B}: give one list, or one per batch entry")
    docs = tuple(_one_list(np.asarray(c).tolist() if isinstance(c, np.ndarray) else c, S_total) for c in lists)
    if all(len(c) == 2 for c in docs):
        return SINGLE
    if len(set(docs)) == 1:
        docs = docs[:1]
    return Docs(docs)


def refuse_not_causal_self(causal, Sq_total: int, Sk_total: int, name: str = "cu_doclens"):
    """The document mask is intra-document CAUSAL self-attention (`name`: the argument the refusal names)."""
    if not causal:
        raise NotImplementedError(f"{name} needs causal=True: non-causal documents are not served")
    if Sq_total != Sk_total:
        raise NotImplementedError(f"{name} needs causal=True self-attention: the whole q and k have the same length, got "
                                  f"{Sq_total} and {Sk_total}")


DOCUMENTS = "documents"      # bidirectional="documents": every document is one span


def _span_list(spans, S_total):
    """One list of (s, e) pairs -> a tuple of int pairs, checked: 0 <= s < e <= S_total, sorted, pairwise disjoint."""
    if isinstance(spans, torch.Tensor):
        if spans.dtype.is_floating_point or spans.dtype == torch.bool:
            raise ValueError(f"bidirectional must hold integers, got {spans.dtype}")
        spans = spans.tolist()
    elif isinstance(spans, np.ndarray):
        if spans.dtype.kind not in "iu":
            raise ValueError(f"bidirectional must hold integers, got {spans.dtype}")
        spans = spans.tolist()
    out = []
    for pair in spans:
        pair = pair.tolist() if isinstance(pair, (torch.Tensor, np.ndarray)) else pair
        if not isinstance(pair, (list, tuple)) or len(pair) != 2 or any(isinstance(x, (float, bool)) for x in pair):
            raise ValueError(f"bidirectional must be a list of (start, end) integer pairs, got {pair!r}")
        s, e = int(pair[0]), int(pair[1])
        if not 0 <= s < e <= S_total:
            raise ValueError(f"bidirectional span ({s}, {e}) must satisfy 0 <= start < end <= {S_total}")
        if out and s < out[-1][1]:
            raise ValueError(f"bidirectional spans must be sorted and pairwise disjoint: ({s}, {e}) follows {out[-1]}")
        out.append((s, e))
    return tuple(out)


def _span_lists(bidirectional, B, S_total):
    """`bidirectional` (not None, not "documents") -> a tuple of one checked list or B of them."""
    if isinstance(bidirectional, torch.Tensor):
        if bidirectional.device.type != "cpu":
            raise ValueError(f"bidirectional must be host data (a Python sequence or a CPU integer tensor), got a tensor on "
                             f"{bidirectional.device}: the planner reads it without a device sync")
        if bidirectional.dim() not in (2, 3) or bidirectional.shape[-1] != 2:
            raise ValueError(f"bidirectional as a tensor must have shape (n, 2) or (B, n, 2), got {tuple(bidirectional.shape)}")
        nested = bidirectional.dim() == 3
        lists = list(bidirectional) if nested else [bidirectional]
    elif isinstance(bidirectional, str):
        raise ValueError(f"bidirectional must be a list of (start, end) pairs or {DOCUMENTS!r}, got {bidirectional!r}")
    else:
        try:
            lists = list(bidirectional)
        except TypeError:
            raise ValueError(f"bidirectional must be a list of (start, end) pairs or {DOCUMENTS!r}, got {bidirectional!r}") from None
        for t in lists:
            if isinstance(t, torch.Tensor) and t.device.type != "cpu":
                raise ValueError(f"bidirectional must be host data, got a tensor on {t.device}")

        def is_list_of_pairs(x):       # an empty list, or one whose first element is itself a pair
            if isinstance(x, (torch.Tensor, np.ndarray)):
                return x.ndim == 2
            return isinstance(x, (list, tuple)) and (len(x) == 0 or isinstance(x[0], (list, tuple, torch.Tensor, np.ndarray)))
        nested = len(lists) > 0 and is_list_of_pairs(lists[0])
        if not nested:
            lists = [lists]
    if nested and len(lists) != B:
        raise ValueError(f"bidirectional holds {len(lists)} lists for a batch of {B}: give one list, or one per batch entry")
    return tuple(_span_list(x, S_total) for x in lists)


def parse_plan(cu_doclens, bidirectional, B: int, S_total: int):
    """(`cu_doclens`, `bidirectional`) -> what parse() returns -- None, SINGLE or the checked lists -- when no span is on, else a
    Spans plan.  Off: None, an empty list, or spans that all have length 1: EXACTLY parse(cu_doclens), whatever that is.
    bidirectional="documents": every document of cu_doclens is one span (without cu_doclens: the whole sequence).  A plan that
    was parsed before is handed back as it is.  ValueError: parse()'s, and a list that is unsorted or overlapping, an empty or
    out-of-range span, a span that crosses a document boundary, a device tensor, B lists for another B, another string."""
    docs = parse(cu_doclens, B, S_total)
    if bidirectional is None or spans_of(docs) is not None:
        return docs
    lists = ((0, S_total),) if (docs is None or docs is SINGLE) else tuple(docs)
    if isinstance(bidirectional, str) and bidirectional == DOCUMENTS:
        spans = tuple(tuple(zip(cu[:-1], cu[1:])) for cu in lists)
    else:
        spans = _span_lists(bidirectional, B, S_total)
    n = max(len(lists), len(spans))
    lists = lists * n if len(lists) == 1 else lists
    spans = spans * n if len(spans) == 1 else spans
    for cu, sp in zip(lists, spans):
        for s, e in sp:
            if int(starts_of(cu, s, 1)[0]) != int(starts_of(cu, e - 1, 1)[0]):
                raise ValueError(f"bidirectional span ({s}, {e}) crosses a document boundary of cu_doclens: every span must lie "
                                 f"inside one document")
    spans = tuple(tuple((s, e) for s, e in sp if e - s > 1) for sp in spans)      # (a span of one position changes nothing)
    if not any(spans):
        return docs
    if len(set(zip(lists, spans))) == 1:
        lists, spans = lists[:1], spans[:1]
    return Spans(lists, spans)


def his_of(spans, lo: int, n: int) -> np.ndarray:
    """hi(i) for the global positions i in [lo, lo + n): the end of the span that holds i, i + 1 where none does."""
    pos = np.arange(lo, lo + n, dtype=np.int64)
    hi = pos + 1
    for s, e in spans:
        a, b = max(s, lo) - lo, min(e, lo + n) - lo
        if a < b:
            hi[a:b] = e
    return hi


def span_block_arrays(cu, spans, row0: int, n_rows: int, key0: int, n_keys: int):
    """(row_lo, row_hi, key_lo, key_hi) int32 of the launch whose rows are the global positions [row0, row0 + n_rows) and
    whose keys are [key0, key0 + n_keys), for ONE list with its spans; None when no row sees a key under
    start(i) <= j < hi(i).  The diagonal lies in row_hi: the launch is not causal."""
    row_lo = np.clip(starts_of(cu, row0, n_rows) - key0, 0, n_keys)
    row_hi = np.clip(his_of(spans, row0, n_rows) - key0, 0, n_keys)
    if not np.any(row_lo < row_hi):
        return None
    keys = np.arange(n_keys, dtype=np.int64)
    # monotone bounds: the rows that see key j are the leading ones with row_lo <= j less the leading ones with row_hi <= j
    key_hi = np.searchsorted(row_lo, keys, side="right")
    key_lo = np.searchsorted(row_hi, keys, side="right")
    return tuple(a.astype(np.int32) for a in (row_lo, row_hi, key_lo, key_hi))


def span_empty_arrays(n_rows: int, n_keys: int):
    """The four arrays of a batch entry that sees nothing in a launch another entry needs."""
    return (np.full(n_rows, n_keys, dtype=np.int32), np.zeros(n_rows, dtype=np.int32),
            np.full(n_keys, n_rows, dtype=np.int32), np.zeros(n_keys, dtype=np.int32))


def starts_of(cu, lo: int, n: int) -> np.ndarray:
    """start(i) for the global positions i in [lo, lo + n): the first position of the document that holds i."""
    cu = np.asarray(cu, dtype=np.int64)
    pos = np.arange(lo, lo + n, dtype=np.int64)
    return cu[np.searchsorted(cu, pos, side="right") - 1]


def block_arrays(cu, row0: int, n_rows: int, key0: int, n_keys: int):
    """(row_lo, key_hi) int32 of the launch whose rows are the global positions [row0, row0 + n_rows) and whose keys are
    [key0, key0 + n_keys), for ONE list; None when no row sees a key under start(i) <= j <= i."""
    start = starts_of(cu, row0, n_rows)
    pos = np.arange(row0, row0 + n_rows, dtype=np.int64)
    lo_g = np.maximum(start, key0)
    if not np.any(lo_g <= np.minimum(pos, key0 + n_keys - 1)):
        return None
    row_lo = np.clip(start - key0, 0, n_keys).astype(np.int32)
    # monotone row_lo: the rows that see key j are the leading ones with row_lo <= j
    key_hi = np.searchsorted(row_lo, np.arange(n_keys, dtype=np.int64), side="right").astype(np.int32)
    return row_lo, key_hi


def empty_arrays(n_rows: int, n_keys: int):
    """The arrays of a batch entry that sees nothing in a launch another entry needs: every row_lo = n_keys."""
    return np.full(n_rows, n_keys, dtype=np.int32), np.zeros(n_keys, dtype=np.int32)


class DocCall:
    """The document arrays of one call (a forward or a backward): `add` every launch's ranges first, `upload` once, then
    `doc(key)` gives the `doc=(row_lo, key_hi)` keyword of a launch (device int32 tensors, (n,) for one list or (B, n)), or
    None for a launch in which nothing is visible -- which the caller drops.  A plan with spans (Spans) gives the four arrays
    (row_lo, row_hi, key_lo, key_hi) instead, which a launch takes as `span=`: `kw(key)` is the keyword either way, and
    `causal(key, causal)` the launch's causal flag (a span launch holds the diagonal in row_hi)."""

    def __init__(self, docs):
        self.docs = docs
        self._host = {}            # key -> (row_lo (L, n_rows), key_hi (L, n_keys)) | None
        self._dev = {}

    def add(self, key, row0: int, n_rows: int, key0: int, n_keys: int) -> bool:
        """Plans the launch `key`; False: nothing visible for any batch entry."""
        spans = spans_of(self.docs)
        if spans is None:
            per = [block_arrays(cu, row0, n_rows, key0, n_keys) for cu in self.docs]
            empty = empty_arrays
        else:
            per = [span_block_arrays(cu, sp, row0, n_rows, key0, n_keys) for cu, sp in zip(self.docs, spans)]
            empty = span_empty_arrays
        if all(p is None for p in per):
            self._host[key] = None
            return False
        per = [empty(n_rows, n_keys) if p is None else p for p in per]
        self._host[key] = tuple(np.stack([p[i] for p in per]) for i in range(len(per[0])))
        return True

    def visible(self, key) -> bool:
        return self._host[key] is not None

    def upload(self, device):
        """One host buffer, one copy."""
        live = [(k, v) for k, v in self._host.items() if v is not None]
        if not live:
            return self
        flat = np.concatenate([a.reshape(-1) for _, v in live for a in v])
        buf = torch.from_numpy(flat)
        if torch.device(device).type != "cpu":
            buf = buf.to(device)
        off = 0
        for k, v in live:
            views = []
            for a in v:
                t = buf[off:off + a.size]
                views.append(t if a.shape[0] == 1 else t.view(a.shape))
                off += a.size
            self._dev[k] = tuple(views)
        return self

    def doc(self, key):
        return self._dev.get(key)

    def kw(self, key) -> dict:
        """The keyword of the launch `key`: doc=(row_lo, key_hi), or span=(row_lo, row_hi, key_lo, key_hi) under a plan with spans."""
        return {"doc" if spans_of(self.docs) is None else "span": self._dev.get(key)}

    def causal(self, key, causal: bool) -> bool:
        return bool(causal) and spans_of(self.docs) is None


def whole_call(docs, S: int, device) -> DocCall:
    """The one-block call: rows and keys are the whole sequence."""
    call = DocCall(docs)
    call.add(0, 0, S, 0, S)
    return call.upload(device)


def ring_call(docs, S: int, P: int, r: int, device) -> DocCall:
    """The basic ring on ring rank r of P, S rows each: step s sees the K/V of ring rank kr = r - s, keys [kr S, (kr + 1) S);
    under causal only the steps s <= r compute.  Launch keys are the steps.  Under a plan with spans a block ABOVE the diagonal
    (kr > r, step = r - kr + P) can be live too -- a span that straddles a shard boundary -- so every step is planned."""
    call = DocCall(docs)
    for step in (range(r + 1) if spans_of(docs) is None else range(P)):
        call.add(step, r * S, S, ((r - step) % P) * S, S)
    return call.upload(device)


def ring_visible(docs, S: int, rank: int, step: int, P: int = 0) -> bool:
    """Does ring rank `rank` launch step `step`?  Host arithmetic any rank can do for any other: the block is visible iff
    the first row of the rank's shard starts its document in front of the block's last key (start(rank S) < (kr + 1) S).
    Under a plan with spans (`P`, the ring degree, is then needed: kr = (rank - step) mod P may lie above the diagonal) both
    bounds count: below the diagonal the same test (the right bound of every row reaches past the block), above it the block is
    visible iff the last row of the shard sees past the block's first key (hi((rank + 1) S - 1) > kr S)."""
    spans = spans_of(docs)
    if spans is None:
        if step > rank:
            return False
        kr = rank - step
        return any(int(starts_of(cu, rank * S, 1)[0]) < (kr + 1) * S for cu in docs)
    assert P > 0, "ring_visible under spans needs the ring degree"
    kr = (rank - step) % P
    if kr <= rank:
        return any(int(starts_of(cu, rank * S, 1)[0]) < (kr + 1) * S for cu in docs)
    return any(int(his_of(sp, (rank + 1) * S - 1, 1)[0]) > kr * S for sp in spans)


def spans_cross_shards(docs, S: int, P: int) -> bool:
    """Does some span straddle a shard boundary of the basic ring (P shards of S positions)?  Then a block above the diagonal is
    live and the document ring's schedule, which moves K/V downwards only, does not serve the call."""
    return any((s // S) != ((e - 1) // S) for sp in (spans_of(docs) or ()) for s, e in sp)


class SpanRingPlan:
    """The live blocks of a basic-ring call under spans as ring rank `rank` sees them, in the terms of the planned direct
    transport (ring/window_blocks.py: WindowPlan): `steps` this rank launches, ascending; `recv` / `send`, both ends of every K/V
    transfer, derived from the one function ring_visible; key_extent(rank, step) for the dK/dV return (a live block carries
    gradients for the whole shard)."""

    def __init__(self, docs, S: int, P: int, rank: int):
        self.docs, self.S, self.P, self.rank = docs, S, P, rank
        self.steps = [s for s in range(P) if ring_visible(docs, S, rank, s, P)]
        self.recv = [s for s in self.steps if s > 0]
        self.send = [s for s in range(1, P) if ring_visible(docs, S, (rank + s) % P, s, P)]

    def key_extent(self, rank: int, step: int):
        return slice(0, self.S) if ring_visible(self.docs, self.S, rank, step, self.P) else None
