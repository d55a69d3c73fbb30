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
"""
import numpy as np
import torch

SINGLE = "single"        # parse(): the list is one document -- exactly the call without it


class Docs(tuple):
    """What parse() returns for a list it has checked: a tuple of one list (shared by the batch) or B lists, each a tuple of
    ints.  parse() hands it back as it is, so a layer may parse once and pass the result down."""


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


def refuse_not_causal_self(causal, Sq_total: int, Sk_total: int):
    """The document mask is intra-document CAUSAL self-attention."""
    if not causal:
        raise NotImplementedError("cu_doclens needs causal=True: non-causal documents are not served")
    if Sq_total != Sk_total:
        raise NotImplementedError(f"cu_doclens needs causal=True self-attention: the whole q and k have the same length, got "
                                  f"{Sq_total} and {Sk_total}")


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
    None for a launch in which nothing is visible -- which the caller drops."""

    def __init__(self, docs):
        self.docs = docs
        self._host = {}            # key -> (row_lo (L, n_rows), key_hi (L, n_keys)) | None
        self._dev = {}

    def add(self, key, row0: int, n_rows: int, key0: int, n_keys: int) -> bool:
        """Plans the launch `key`; False: nothing visible for any batch entry."""
        per = [block_arrays(cu, row0, n_rows, key0, n_keys) for cu in self.docs]
        if all(p is None for p in per):
            self._host[key] = None
            return False
        per = [empty_arrays(n_rows, n_keys) if p is None else p for p in per]
        self._host[key] = (np.stack([p[0] for p in per]), np.stack([p[1] for p in per]))
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


def whole_call(docs, S: int, device) -> DocCall:
    """The one-block call: rows and keys are the whole sequence."""
    call = DocCall(docs)
    call.add(0, 0, S, 0, S)
    return call.upload(device)


def ring_call(docs, S: int, P: int, r: int, device) -> DocCall:
    """The basic ring on ring rank r of P, S rows each: step s sees the K/V of ring rank kr = r - s, keys [kr S, (kr + 1) S);
    under causal only the steps s <= r compute.  Launch keys are the steps."""
    call = DocCall(docs)
    for step in range(r + 1):
        call.add(step, r * S, S, (r - step) * S, S)
    return call.upload(device)


def ring_visible(docs, S: int, rank: int, step: int) -> bool:
    """Does ring rank `rank` launch step `step`?  Host arithmetic any rank can do for any other: the block is visible iff
    the first row of the rank's shard starts its document in front of the block's last key (start(rank S) < (kr + 1) S)."""
    if step > rank:
        return False
    kr = rank - step
    return any(int(starts_of(cu, rank * S, 1)[0]) < (kr + 1) * S for cu in docs)
