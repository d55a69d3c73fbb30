"""Block plan of a GLOBAL sliding window on the contiguous ("basic") ring.  Pure Python: no torch, no device.

Global positions are 0 ... S-1; row i sees key j iff  i - wl <= j <= i + wr  (a negative bound is unbounded; with `causal`
also j <= i).  Ring rank r holds rows [r c, (r+1) c) and meets, at ring step s, the K/V of rank src = (r - s) mod P.  With
shift = (r - src) c and right = 0 if causal else wr the block's mask in LOCAL indices is

    i + shift - wl <= j <= i + shift + right          (each side only where its bound is >= 0)

which the block kernels take as `causal` / `window` plus the diagonal shift of the C ABI (USP_ATTN_SHIFT, include/usp_hip.h).
The reference hands the same `window_size` to every block (yunchang/ring/ring_flash_attn.py:36-48): a different function,
which is why nothing here is modelled on it.

`plan_block` classifies one (rank, step) block -- empty, full, or a launch description in which a bound that does not bite is
dropped (a full block is a plain non-causal launch, eligible for every kernel family) and a right bound of 0 is expressed as
`causal=True` plus the shift (the causal instantiations serve it) -- and `recv_steps` / `send_steps` derive both ends of every
K/V transfer from that one function: rank r receives the K/V of rank r - s exactly when block (r, s) is not empty, and sends
its own to rank r + s exactly when block ((r + s) mod P, s) is not.
"""
from typing import NamedTuple, Optional, Tuple


class Block(NamedTuple):
    """One non-empty block, as launched: `causal`, `window` ((left, right) | None) and `shift` (None: the launch carries no
    shift -- a full block, or the diagonal block of step 0) are the kernel arguments; `keys` / `rows` are the half-open
    ranges of local key rows that carry gradients and of local query rows that see a key."""
    causal: bool
    window: Optional[Tuple[int, int]]
    shift: Optional[int]
    keys: Tuple[int, int]
    rows: Tuple[int, int]

    @property
    def full(self) -> bool:
        return not self.causal and self.window is None

    def launch_kw(self) -> dict:
        """The keywords a block backend's fwd / bwd take beside `causal` (absent where off, so a backend written before
        either keyword existed still serves the blocks that do not need it)."""
        kw = {}
        if self.window is not None:
            kw["window"] = self.window
        if self.shift is not None:
            kw["shift"] = self.shift
        return kw


def check_plan_args(P: int, c: int, wl: int, wr: int):
    if P < 1 or c < 1:
        raise ValueError(f"ring degree {P} and chunk {c} must be positive")
    if max(abs(int(wl)), abs(int(wr))) >= 1 << 30 or P * c >= 1 << 30:
        raise ValueError("window bounds and the sequence length must stay below 2^30")


def plan_block(P: int, c: int, causal: bool, wl: int, wr: int, rank: int, step: int) -> Optional[Block]:
    """The block ring rank `rank` meets at ring step `step`; None when no row of it sees a key."""
    src = (rank - step) % P
    shift = (rank - src) * c
    right = 0 if causal else wr
    has_l, has_r = wl >= 0, right >= 0
    if (has_l and shift - wl > c - 1) or (has_r and c - 1 + shift + right < 0):
        return None
    left_bites = has_l and c - 1 + shift - wl > 0
    right_bites = has_r and shift + right < c - 1
    keys = (max(0, shift - wl) if has_l else 0, min(c, c + shift + right) if has_r else c)
    rows = (max(0, -shift - right) if has_r else 0, min(c, c - shift + wl) if has_l else c)
    as_causal = right_bites and right == 0
    win_r = -1 if (not right_bites or as_causal) else right
    # (under `causal` the kernels cap the right bound at 0 whatever the window says: (wl, 0) states it)
    window = (wl, 0 if as_causal else win_r) if left_bites else ((-1, win_r) if win_r >= 0 else None)
    bounded = as_causal or window is not None
    return Block(as_causal, window, shift if (bounded and shift != 0) else None, keys, rows)


def compute_steps(P: int, c: int, causal: bool, wl: int, wr: int, rank: int):
    """Ring steps of `rank` whose block is not empty, ascending (step 0 never is: every row sees its own key)."""
    return [s for s in range(P) if plan_block(P, c, causal, wl, wr, rank, s) is not None]


def recv_steps(P: int, c: int, causal: bool, wl: int, wr: int, rank: int):
    """Steps s >= 1 whose K/V (owned by rank - s) `rank` needs."""
    return [s for s in compute_steps(P, c, causal, wl, wr, rank) if s > 0]


def send_steps(P: int, c: int, causal: bool, wl: int, wr: int, rank: int):
    """Steps s >= 1 at which rank + s needs the K/V of `rank`."""
    return [s for s in range(1, P) if plan_block(P, c, causal, wl, wr, (rank + s) % P, s) is not None]


class WindowPlan:
    """The plan of one call as one rank sees it."""

    def __init__(self, P: int, c: int, causal: bool, wl: int, wr: int, rank: int):
        check_plan_args(P, c, wl, wr)
        self.P, self.c, self.causal, self.wl, self.wr, self.rank = P, c, bool(causal), int(wl), int(wr), rank
        self._args = (P, c, self.causal, self.wl, self.wr)
        self.steps = compute_steps(*self._args, rank)
        self.recv = [s for s in self.steps if s > 0]
        self.send = send_steps(*self._args, rank)

    def block(self, step: int, rank: Optional[int] = None) -> Optional[Block]:
        return plan_block(*self._args, self.rank if rank is None else rank, step)

    def key_extent(self, rank: int, step: int):
        """None | slice of local key rows whose gradients the block of `step` on ring rank `rank` carries."""
        blk = self.block(step, rank)
        return None if blk is None else slice(*blk.keys)
