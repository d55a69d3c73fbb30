"""ONE causal block issued in pieces: what the basic and the zigzag ring -- the same single block at ring degree 1 -- do when the
caller (the head-group pipeline at ulysses degree 2, hybrid/async_attn_layer.py) has exchanges in flight around the block:

    first     the block starts on the rows this rank already holds, the rest follows behind the exchange (self_chunk_mode);
    tail      the block runs in row pieces and every piece's output leaves while the next one computes (tails_mode);
    dq_first  the backward issues its dQ launch first and dq travels beside the dK/dV launch.

Launches and allocations only: the backend (interleavable: the caller has transfers in flight by definition) arrives from the
ring function, nothing here asks torch.distributed for anything.  Unlike step 0 of a ring (degree > 1) every row is final behind
its last launch, so there is no fp32 `acc` for rows that are final at once and no fp32 dQ accumulator at all: the kernels round
in their epilogues (`dq16` / `dk16` / `dv16`).  Results equal the one launch up to fp32 summation order."""
import torch


def split_first_forward(be, u, selfs, full, wait, scale):
    """The block started on the self chunk.  `selfs` = (q, k, v) of this rank's own rows (views of the exchange's send buffer),
    `full` = (q, k, v) over all 2c rows (views of the receive buffer, valid behind `wait()`); ulysses rank u = 0 owns rows
    [0, c), u = 1 rows [c, 2c).  Returns (out, lse) as the ring forward would."""
    qs, ks, vs = selfs
    q, k, v = full
    B, S, hq, D = q.shape
    c = S // 2
    out = torch.empty((B, S, hq, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, hq, S), dtype=torch.float32, device=q.device)
    if u == 0:       # own rows [0, c): they see own keys only -- complete and final at once
        be.fwd(qs, ks, vs, scale, True, lse[:, :, :c], out[:, :c])
        wait()
        be.fwd(q[:, c:], k, v, scale, True, lse[:, :, c:], out[:, c:])          # c rows x 2c keys, bottom-right causal
    else:            # own rows [c, 2c): the diagonal block now, the peer's keys merged in behind the exchange
        acc = torch.empty((B, c, hq, D), dtype=torch.float32, device=q.device)
        be.fwd(qs, ks, vs, scale, True, lse[:, :, c:], None, acc, False, 0, 0)
        wait()
        be.fwd(q[:, c:], k[:, :c], v[:, :c], scale, False, lse[:, :, c:], out[:, c:], acc, True, 0, c)
        be.fwd(q[:, :c], k[:, :c], v[:, :c], scale, True, lse[:, :, :c], out[:, :c])
    return out, lse


def split_first_backward(be, u, do_self, do_full, wait, q, k, v, o, lse, scale):
    """The backward of the same block: K, V, out and the LSE are there (saved), only dO travels -- the rows this rank owns
    start at once, the peer's rows follow behind the exchange; dK / dV accumulate in fp32 across the two launches and are
    rounded by the last one that touches a row.  Returns (dq, dk, dv) in q.dtype."""
    B, S, hq, D = q.shape
    kvh = k.shape[2]
    c = S // 2
    dev = q.device
    delta = torch.empty((B, hq, S), dtype=torch.float32, device=dev)
    dq = torch.empty((B, S, hq, D), dtype=q.dtype, device=dev)
    dk = torch.empty((B, S, kvh, D), dtype=k.dtype, device=dev)
    dv = torch.empty_like(dk)
    dk32 = torch.empty((B, S, kvh, D), dtype=torch.float32, device=dev)
    dv32 = torch.empty_like(dk32)
    if u == 0:       # rows [0, c) x keys [0, c) first; then rows [c, 2c) x all keys on top
        be.delta(do_self, o[:, :c], delta[:, :, :c])
        dk32[:, c:].zero_()
        dv32[:, c:].zero_()
        be.bwd(do_self, q[:, :c], k[:, :c], v[:, :c], lse[:, :, :c], delta[:, :, :c], None, dk32[:, :c], dv32[:, :c], scale, True,
               dq16=dq[:, :c])
        wait()
        be.delta(do_full[:, c:], o[:, c:], delta[:, :, c:])
        be.bwd(do_full[:, c:], q[:, c:], k, v, lse[:, :, c:], delta[:, :, c:], None, dk32, dv32, scale, True,
               accum_dk=True, accum_dv=True, dq16=dq[:, c:], dk16=dk, dv16=dv)
    else:            # rows [c, 2c) x all keys first (3/4 of the block); then rows [0, c) x keys [0, c) on top
        be.delta(do_self, o[:, c:], delta[:, :, c:])
        be.bwd(do_self, q[:, c:], k, v, lse[:, :, c:], delta[:, :, c:], None, dk32, dv32, scale, True, dq16=dq[:, c:])
        wait()
        be.delta(do_full[:, :c], o[:, :c], delta[:, :, :c])
        be.bwd(do_full[:, :c], q[:, :c], k[:, :c], v[:, :c], lse[:, :, :c], delta[:, :, :c], None, dk32[:, :c], dv32[:, :c], scale,
               True, accum_dk=True, accum_dv=True, dq16=dq[:, :c], dk16=dk[:, :c], dv16=dv[:, :c])
        be.cast(dk[:, c:], dk32[:, c:])              # keys [c, 2c) got gradients from the first launch only
        be.cast(dv[:, c:], dv32[:, c:])
    return dq, dk, dv


def tail_last_forward(be, q, k, v, scale, n, emit):
    """The block in row pieces: piece j of the front chunk, piece j of the back chunk (each a bottom-right-aligned causal
    launch over the keys its rows see), then `emit(j, out)` -- the piece's output exchange runs beside the next piece's
    launches.  Same rows x keys as one launch; returns (out, lse)."""
    B, S, hq, D = q.shape
    c = S // 2
    out = torch.empty((B, S, hq, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, hq, S), dtype=torch.float32, device=q.device)
    for j in range(n):
        for ch in (0, 1):
            a, b = ch * c + j * c // n, ch * c + (j + 1) * c // n
            if b > a:
                be.fwd(q[:, a:b], k[:, :b], v[:, :b], scale, True, lse[:, :, a:b], out[:, a:b])
        emit(j, out)
    return out, lse


def tail_last_backward(be, dout, q, k, v, o, lse, scale, dq_first):
    """... and its backward: delta, the dQ launch (rounded in its epilogue), `dq_first(dq)` -- dq travels beside the dK/dV launch
    --, the dK/dV launch.  Returns (dq, dk, dv) in q.dtype."""
    B, S, hq, D = q.shape
    delta = torch.empty((B, hq, S), dtype=torch.float32, device=q.device)
    dq = torch.empty((B, S, hq, D), dtype=q.dtype, device=q.device)
    dk = torch.empty((B, S, k.shape[2], D), dtype=k.dtype, device=q.device)
    dv = torch.empty_like(dk)
    be.delta(dout, o, delta)
    be.bwd(dout, q, k, v, lse, delta, None, None, None, scale, True, dq16=dq, only="dq")
    dq_first(dq)
    be.bwd(dout, q, k, v, lse, delta, None, None, None, scale, True, dk16=dk, dv16=dv, only="dkdv")
    return dq, dk, dv


def refuse_sinks(sinks, pieces):
    """The pieces open a row range with more than one launch without merge_in (split_first_forward, tail_last_forward): a sink
    riding on those would not be the one block's.  Only the head-group pipeline asks for pieces."""
    if sinks is not None and pieces:
        raise NotImplementedError("sinks is not supported with a block issued in pieces (first / tail / dq_first: the head-group "
                                  "pipeline of AsyncLongContextAttention): use LongContextAttention")


def forward_in_pieces(be, q, k, v, scale, first=None, tail=None):
    """A ring forward's degree-1 route for `first` = (u, (q, k, v) of the own rows, wait) or `tail` = (n, emit).  The split
    owns the block where both are given."""
    if first is not None:
        u, own, wait = first
        return split_first_forward(be, u, own, (q, k, v), wait, scale)
    return tail_last_forward(be, q, k, v, scale, *tail)


def backward_in_pieces(be, dout, q, k, v, out, lse, scale, first=None, dq_first=None):
    """A ring backward's degree-1 route for `first` = (u, dO of the own rows, wait) or `dq_first`.  The split owns the block
    where both are given: `dq_first` is then never called, dq comes back with dk and dv."""
    if first is not None:
        u, do_own, wait = first
        return split_first_backward(be, u, do_own, dout, wait, q, k, v, out, lse, scale)
    return tail_last_backward(be, dout, q, k, v, out, lse, scale, dq_first)
