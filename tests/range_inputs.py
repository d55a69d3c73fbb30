"""Value-range inputs: q, k, v, dout outside N(0,1) and softmax scales other than D^-0.5.

Every other input family of this tree (N(0,1), tests/needle_inputs.py) stays inside one envelope: |score * log2(e)| below
24, K * scale * log2(e) below 1, softmax_scale = D^-0.5.  The kernels are not neutral to values: each folds the scale in
another place (one FMA per score and a deferred-max threshold kThr / c in the forwards, a per-element FMA in the 64-row
forward and dQ kernels, tanh_k2 = 2 c / cap under softcap, the start constant of the S chain in the 64-row dK/dV kernel).
Four families, plain numpy, deterministic from a seed, every value rounded to the 16-bit type at the end (the fp64
reference and the kernels read the same numbers):

- `offset`: N(0,1) plus `nch` outlier channels: constant `amp` on q, amp * (1 + jit * N(0,1)) on k.  Every score of a row
  carries a common offset of nch * amp^2 * scale nat (51 nat at amp 24, D 128) that cancels in the softmax -- unless an
  operand was rounded after the scale was folded into it: then the error of channel d is q_d k_d c 2^-9 per key, the
  same for every row, and a whole dK / dV row is off by a factor.
- `scaled`: scales other than D^-0.5.  Exact pairs (q 2^j, k, scale 2^-j) and (q, k 2^j, scale 2^-j) are the same
  problem in exact arithmetic (powers of two); the reference is the fp64 result of the UNSCALED problem, the gradient
  the scaled operand owns is compared after multiplication by 2^j.  Independent scales (0.02, 0.3, 1.0) shrink or grow
  q by a power of two so that the scores stay within +-15 nat.
- `steps` (forward only): one key per 64-key tile is aligned with the query rows of a block; its score (log2 units)
  changes from tile to tile by a chosen amount, multiplied per row by a factor that varies inside every wave -- some
  rows of a wave jump past the forwards' deferred-max threshold (kThr = 8) and others do not.
- `fp16_edge`: fp16 with softmax_scale 5.5 / 5.6 (scale * log2(e) = 7.93 / 8.08) and one K channel at +-12288.

`ref` of a case holds the operands of the problem the fp64 reference solves (for an exact pair: the unscaled problem),
`mul` the factor that turns a result of the launched problem into one of the reference problem (2^j on the gradient of
the scaled operand), `norm` a power of two (per tensor, or per channel of the head dim) both sides are multiplied by before they are judged
(fp16_edge only: its dout is 2^-6 N(0,1)).
"""
from types import SimpleNamespace
from typing import NamedTuple, Optional, Tuple

import numpy as np

from golden_util import round_to

LOG2E = 1.4426950408889634
TILE = 64


class Case(NamedTuple):
    id: str
    kind: str                             # offset | pair | scale | steps | edge
    Sq: int
    Sk: int
    Hq: int
    Hkv: int
    D: int
    causal: bool
    dt: str
    family: Optional[str]                 # "row64" | "wave32" | None (the library's own dispatch)
    par: Tuple = ()                       # parameters of the kind (see the generators)
    scale: Optional[float] = None         # None: D^-0.5
    softcap: Optional[float] = None
    k_splits: int = 0
    splits: Tuple[int, int] = (0, 0)
    dkdv_heads: int = 0
    seed: int = 0


def _normals(c, rs):
    return [rs.standard_normal(s) for s in [(1, c.Sq, c.Hq, c.D), (1, c.Sk, c.Hkv, c.D), (1, c.Sk, c.Hkv, c.D),
                                            (1, c.Sq, c.Hq, c.D)]]


def _finish(c, q, k, v, do, scale, ref=None, mul=None, norm=None):
    q, k, v, do = (round_to(np.asarray(x, dtype=np.float32), c.dt) for x in (q, k, v, do))
    ns = SimpleNamespace(q=q, k=k, v=v, do=do, scale=float(scale), mul=dict(mul or {}), norm=dict(norm or {}))
    ns.ref = SimpleNamespace(q=q.astype(np.float64), k=k.astype(np.float64), scale=float(scale)) if ref is None else ref(q, k)
    return ns


def offset_channels(nch, D):
    """The outlier channels: 17 first (the case the family was designed on), the others spread over the head dim."""
    return [(17 + i * (D // 4 + 3)) % D for i in range(nch)]


def make_offset(c):
    """par = (amp, nch, jit, do_mul, do_mean): dout = do_mul * (N(0,1) + do_mean * s) with one sign vector s (D,) for all
    rows.  The common part makes the rows' contributions to a key's dK / dV row add up coherently: the row grows past
    atol / rtol, where an error that is a FACTOR on the whole row is judged by rtol alone, while the honest rounding
    errors (absolute, ~ do_mul) stay where they were."""
    amp, nch, jit, do_mul, do_mean = c.par
    rs = np.random.RandomState(2000 + c.seed)
    q, k, v, do = _normals(c, rs)
    do = do + do_mean * np.where(rs.rand(c.D) < 0.5, -1.0, 1.0)
    for ch in offset_channels(nch, c.D):
        q[..., ch] = amp
        k[..., ch] = amp * (1.0 + jit * rs.standard_normal(k.shape[:-1]))
    return _finish(c, q, k, v, do * do_mul, c.D ** -0.5 if c.scale is None else c.scale)


def make_pair(c):
    """par = (side, j[, j_other, do_mul]): operand `side` ("q" / "k") times 2^j, the other one times 2^j_other (default
    1), scale times 2^-(j + j_other).  The reference problem divides the ROUNDED operands by the same powers of two
    (exact in fp64) and keeps D^-0.5: where a scaled value leaves the 16-bit type's normal range, both sides still read
    the same numbers."""
    side, j = c.par[0], c.par[1]
    jo = c.par[2] if len(c.par) > 2 else 0
    do_mul = c.par[3] if len(c.par) > 3 else 1.0
    rs = np.random.RandomState(3000 + c.seed)
    q, k, v, do = _normals(c, rs)
    jq, jk = (j, jo) if side == "q" else (jo, j)
    s0 = c.D ** -0.5

    def ref(q16, k16):
        return SimpleNamespace(q=q16.astype(np.float64) * 2.0 ** -jq, k=k16.astype(np.float64) * 2.0 ** -jk, scale=s0)
    return _finish(c, q * 2.0 ** jq, k * 2.0 ** jk, v, do * do_mul, s0 * 2.0 ** -(jq + jk), ref,
                   dict(dq=2.0 ** jq, dk=2.0 ** jk))


def q_mul_for(scale, D, nat=3.0):
    """The power of two on q that keeps the scores' standard deviation at or below `nat` (5 sigma inside +-15 nat)."""
    return 2.0 ** np.floor(np.log2(nat / (np.sqrt(D) * scale)))


def make_scale(c):
    """An independent scale `c.scale`; q shrunk or grown by q_mul_for so that the scores stay within +-15 nat.  par =
    (do_mul,) (default 1): dQ = scale dS K carries the rounding error of dS times the scale, 11 x the default one at
    scale 1.0 -- dout is lowered there until the honest model keeps its 2x margin."""
    rs = np.random.RandomState(4000 + c.seed)
    q, k, v, do = _normals(c, rs)
    return _finish(c, q * q_mul_for(c.scale, c.D), k, v, do * (c.par[0] if c.par else 1.0), c.scale)


ROW_MUL = (1.0, 0.75, 0.5, 0.0, 1.25, 1.0, 0.25, 0.875)      # per row r: ROW_MUL[r % 8] -- every wave holds all of them
STEP_CH = 5
STEP_Q = 8.0                                                  # q on the aligned channel of a row with multiplier 1


def step_levels(c):
    """par = ("rise", step) | ("fall", d1, d2): the aligned key's score in log2 units, per 64-key tile, for a row with
    multiplier 1.  Rising: step * t.  Falling: the first tile highest, the second d1 below, the others d2 below."""
    nt = -(-c.Sk // TILE)
    if c.par[0] == "rise":
        return [c.par[1] * t for t in range(nt)]
    _, d1, d2 = c.par
    return [d2, d2 - d1] + [0.0] * (nt - 2)


def step_rows(c):
    """The block of aligned query rows: all but the first and the last eighth of the sequence."""
    return max(1, c.Sq // 8), max(2, c.Sq - c.Sq // 8)


def make_steps(c):
    """Forward only.  Channel STEP_CH of q is STEP_Q * ROW_MUL[r % 8] on the rows of the block and 0 elsewhere; on k it
    is 0 except on one key per tile (at an offset that moves from tile to tile), where it makes the score of a row with
    multiplier 1 the tile's level.  Falling series: v of the second tile's aligned key is 2^11 x N(0,1), so that a weight
    of 2^-15 -- a subnormal of fp16 -- still moves the output by 15 x the tolerance."""
    rs = np.random.RandomState(5000 + c.seed)
    q, k, v, do = _normals(c, rs)
    scale = c.D ** -0.5 if c.scale is None else c.scale
    r0, r1 = step_rows(c)
    q[..., STEP_CH] = 0.0
    k[..., STEP_CH] = 0.0
    rows = np.arange(r0, r1)
    q[:, r0:r1, :, STEP_CH] = (STEP_Q * np.array(ROW_MUL)[rows % 8])[None, :, None]
    v_mul = 2.0 ** 11 if c.par[0] == "fall" else 1.0
    keys = []
    for t, lev in enumerate(step_levels(c)):
        j = min(c.Sk - 1, t * TILE + (7 + 13 * t) % TILE)
        k[:, j, :, STEP_CH] = lev / (STEP_Q * scale * LOG2E)
        if t == 1:
            v[:, j] *= v_mul
        keys.append(j)
    ns = _finish(c, q, k, v, do, scale)
    ns.keys = keys
    return ns


EDGE_CH = 40


def make_edge(c):
    """par = (big_k,): fp16, scale 5.5 / 5.6.  q = 2^-6 N(0,1) (scores of std ~1 nat at these scales); with `big_k`,
    channel EDGE_CH of k is +-12288 (1 + 0.05 N(0,1)) and of q 2^-12 (a normal fp16 number): +-16.5 nat from that
    channel, every value of the fp64 reference finite.  dout = 2^-6 N(0,1): dq = scale dS K reaches 12288 * 5.5 x dS on
    that channel and must stay inside fp16.  The gradients are judged after multiplication by a power of two, both sides
    (`norm`): dk and dv by 2^6 (dout's factor undone), dq by 4 (dQ = scale dS K carries the rounding of dS times 5.5).
    With `big_k`, channel EDGE_CH of dq alone is judged after 2^-10 = 4 * 2^-12: K on that channel is 3 * 2^12 times a
    unit-variance channel, so dq there is a sum scale * sum_j dS_j K_j of terms 2^12 times larger that cancels
    (sum_j dS_j = 0, K nearly constant) -- the honest fp16 rounding of dS alone is 66 x the unscaled bound on that
    channel.  Every other channel keeps the tame case's factor: no element is judged more loosely than its own scale."""
    (big_k,) = c.par
    rs = np.random.RandomState(6000 + c.seed)
    q, k, v, do = _normals(c, rs)
    q *= 2.0 ** -6
    if big_k:
        q[..., EDGE_CH] = 2.0 ** -12
        sign = np.where(rs.rand(*k.shape[:-1]) < 0.5, -1.0, 1.0)
        k[..., EDGE_CH] = sign * 12288.0 * (1.0 + 0.05 * rs.standard_normal(k.shape[:-1]))
    dq_norm = np.full(c.D, 4.0)
    if big_k:
        dq_norm[EDGE_CH] = 2.0 ** -10
    return _finish(c, q, k, v, do * 2.0 ** -6, c.scale, norm=dict(dk=2.0 ** 6, dv=2.0 ** 6, dq=dq_norm))


MAKERS = dict(offset=make_offset, pair=make_pair, scale=make_scale, steps=make_steps, edge=make_edge)


def make(c):
    return MAKERS[c.kind](c)


# ---------------------------------------------------------------------------------------------------------------------
# the reference (oracle.usp_oracle with the explicit scale) and the verdict
# ---------------------------------------------------------------------------------------------------------------------
def packed_reference(c, ns):
    """The per-sequence reference of RI.PACKED: every sequence of PACKED_SEQS is a causal problem of its own."""
    from oracle import usp_oracle as O
    want = {n_: np.zeros(x.shape) for n_, x in (("out", ns.q), ("dq", ns.q), ("dk", ns.k), ("dv", ns.k))}
    want["lse"] = np.zeros((1, c.Hq, c.Sq))
    want["o16"] = np.zeros(ns.q.shape, dtype=np.float32)
    for s0, n in PACKED_SEQS:
        sl = slice(s0, s0 + n)
        ro, rl = O.attention_ref(ns.q[:, sl], ns.k[:, sl], ns.v[:, sl], True, ns.scale)
        want["o16"][:, sl] = round_to(ro.astype(np.float32), c.dt)
        dq, dk, dv = O.block_bwd(ns.do[:, sl], ns.q[:, sl], ns.k[:, sl], ns.v[:, sl], want["o16"][:, sl], rl, ns.scale, True)
        want["out"][:, sl], want["lse"][:, :, sl], want["dq"][:, sl], want["dk"][:, sl], want["dv"][:, sl] = ro, rl, dq, dk, dv
    return want


def reference(c, ns, bwd=True):
    """fp64: out, lse of the reference problem and, with `bwd`, the block backward (exact lse, delta from the 16-bit-rounded
    out) -- O.attention_ref / O.block_bwd; the softcap case goes through tests/attn_ref_torch.py (the oracle has no cap),
    which tests/test_softcap_cpu.py pins against it."""
    from oracle import usp_oracle as O
    r = ns.ref
    if c.softcap:
        import torch

        from attn_ref_torch import ref_bwd, ref_fwd
        tq, tk, tv, tdo = (torch.from_numpy(np.asarray(x, dtype=np.float64)) for x in (r.q, r.k, ns.v, ns.do))
        ro, rl = ref_fwd(tq, tk, tv, r.scale, c.causal, None, c.softcap)
        want = dict(out=ro.numpy(), lse=rl.numpy())
        if bwd:
            o16 = torch.from_numpy(round_to(want["out"].astype(np.float32), c.dt))
            dq, dk, dv, _ = ref_bwd(tdo, tq, tk, tv, o16, rl, r.scale, c.causal, None, c.softcap)
            want.update(dq=dq.numpy(), dk=dk.numpy(), dv=dv.numpy(), o16=o16.numpy())
        return want
    ro, rl = O.attention_ref(r.q, r.k, ns.v, c.causal, r.scale)
    want = dict(out=ro, lse=rl)
    if bwd:
        o16 = round_to(ro.astype(np.float32), c.dt)
        dq, dk, dv = O.block_bwd(ns.do, r.q, r.k, ns.v, o16, rl, r.scale, c.causal)
        want.update(dq=dq, dk=dk, dv=dv, o16=o16)
    return want


def verdicts(c, ns, got, want):
    """needle_inputs.verdicts on `got` x mul against `want`, the reference problem's result (for an exact pair 2^j times
    the launched problem's gradient); both sides x norm.  That is the comparator of every GPU parity file: golden_util.TOL,
    lse 2e-3 + 1e-4 |lse|, every element, and golden_util.long_sum_atol on gradient sums of >= 1000 products -- which the
    offset shapes with Sq * G = 1024 reach for dk and dv: their atol is max(TOL, 8e-3 rms(want)), e.g. 0.070 instead of
    0.05 on offset-51nat, 0.082 instead of 0.01 on offset-fp16 dk, 0.108 on offset-d64-w32 dk (the common part of dout
    raises the rms).  The ratios recorded beside the offset cases are against that bound."""
    import needle_inputs as NI
    g = {n_: np.asarray(x, dtype=np.float64) * (ns.mul.get(n_, 1.0) * ns.norm.get(n_, 1.0)) for n_, x in got.items()}
    return NI.verdicts(g, {n_: want[n_] * ns.norm.get(n_, 1.0) for n_ in g}, c.dt, c.Sq, c.Sk, c.Hq // c.Hkv)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_range.py (tests/test_range_cpu.py asserts the conditions on every one of them)
# ---------------------------------------------------------------------------------------------------------------------
_B, _F = "bfloat16", "float16"
# dout of the offset cases: 2^-4 (N(0,1) + 2 s).  At N(0,1) the honest 16-bit rounding of dS alone costs 1 - 2.7 x the dq
# bound on these inputs (the outlier channel of K multiplies the rounding error of every dS of a row: 24 * scale * sum_j
# err_j); the amplitude is lowered until the honest model keeps a 2x margin, the common part keeps dK / dV rows large
# against atol / rtol (tests/test_range_cpu.py holds both conditions).  Seeds: chosen on the honest model and the
# pre-scaled-K model alone.
DO_MUL, DO_MEAN = 2.0 ** -4, 2.0
OFFSET = [
    # the case the family was designed on: channel 17, amp 24 (51 nat), Sq 512, Sk 64, full attention
    Case("offset-51nat", "offset", 512, 64, 2, 1, 128, False, _B, "row64", (24.0, 1, 0.1, DO_MUL, DO_MEAN), seed=2),
    Case("offset-51nat-w32", "offset", 512, 64, 2, 1, 128, False, _B, "wave32", (24.0, 1, 0.1, DO_MUL, DO_MEAN), seed=2),
    Case("offset-23nat", "offset", 512, 64, 2, 1, 128, False, _B, "row64", (16.0, 1, 0.1, DO_MUL, DO_MEAN), seed=1),
    Case("offset-4ch", "offset", 512, 64, 2, 1, 128, False, _B, "row64", (12.0, 4, 0.1, DO_MUL, DO_MEAN), seed=2),
    Case("offset-causal", "offset", 384, 192, 4, 2, 128, True, _B, "row64", (24.0, 1, 0.1, DO_MUL, DO_MEAN), seed=3),
    Case("offset-fp16", "offset", 512, 64, 2, 1, 128, False, _F, "row64", (24.0, 1, 0.1, DO_MUL, DO_MEAN), seed=3),
    Case("offset-heads1", "offset", 384, 192, 4, 2, 128, True, _B, "row64", (24.0, 1, 0.1, DO_MUL, DO_MEAN), dkdv_heads=1, seed=3),
    Case("offset-heads2", "offset", 384, 192, 4, 2, 128, True, _B, "row64", (24.0, 1, 0.1, DO_MUL, DO_MEAN), dkdv_heads=2, seed=3),
    Case("offset-cuts", "offset", 512, 192, 2, 1, 128, False, _B, "row64", (24.0, 1, 0.1, DO_MUL, DO_MEAN), splits=(2, 2), k_splits=2, seed=2),
    Case("offset-d64-w32", "offset", 512, 64, 2, 1, 64, False, _B, "wave32", (24.0, 1, 0.1, DO_MUL, DO_MEAN)),
    Case("offset-d64-fp16", "offset", 192, 384, 4, 2, 64, True, _F, "wave32", (16.0, 1, 0.1, DO_MUL, DO_MEAN), k_splits=3),
    # softcap 30 on a 51 nat offset: the capped scores sit at 28 nat, where tanh_k2 = 2 c / cap decides the spread
    Case("offset-softcap", "offset", 384, 192, 4, 2, 128, True, _B, None, (24.0, 1, 0.1, DO_MUL, DO_MEAN), softcap=30.0, seed=3),
]
SCALED = [
    Case("pair-q-up", "pair", 384, 192, 4, 2, 128, True, _B, "row64", ("q", 6)),
    Case("pair-q-down", "pair", 192, 384, 2, 1, 128, False, _B, "row64", ("q", -6), k_splits=2),
    Case("pair-k-up", "pair", 512, 512, 2, 1, 128, True, _F, "row64", ("k", 6), splits=(2, 2)),
    Case("pair-k-down", "pair", 64, 192, 4, 2, 128, False, _F, "row64", ("k", -6)),
    Case("pair-q-up-w32", "pair", 192, 384, 4, 2, 64, True, _F, "wave32", ("q", 6), k_splits=3),
    Case("pair-q-down-w32", "pair", 384, 192, 2, 1, 128, True, _B, "wave32", ("q", -6), splits=(2, 2)),
    Case("pair-k-up-w32", "pair", 64, 512, 2, 1, 64, False, _B, "wave32", ("k", 6)),
    Case("pair-k-down-w32", "pair", 512, 64, 4, 2, 128, False, _F, "wave32", ("k", -6), dkdv_heads=1),
    # fp16: k 2^-12, q 2^12, the scale unchanged: K (and K times the scale) sits in the fp16 subnormal range
    Case("pair-k-subnormal", "pair", 384, 192, 2, 1, 128, True, _F, "row64", ("k", -12, 12, 2.0 ** -4)),
    Case("pair-k-subnormal-w32", "pair", 192, 384, 2, 1, 128, False, _F, "wave32", ("k", -12, 12, 2.0 ** -4)),
    Case("scale-0.02", "scale", 384, 384, 4, 2, 128, True, _B, "row64", scale=0.02),
    Case("scale-0.3", "scale", 192, 512, 2, 1, 128, False, _F, "row64", scale=0.3, k_splits=3),
    Case("scale-1.0", "scale", 512, 192, 4, 2, 128, True, _B, "row64", (0.25,), scale=1.0, dkdv_heads=2),
    Case("scale-0.02-w32", "scale", 192, 192, 2, 1, 64, True, _F, "wave32", scale=0.02),
    Case("scale-0.3-w32", "scale", 384, 512, 4, 2, 128, True, _B, "wave32", scale=0.3, splits=(2, 2)),
    Case("scale-1.0-w32", "scale", 512, 384, 2, 1, 64, False, _B, "wave32", (0.25,), scale=1.0, k_splits=2),
]
STEPS = [Case(f"{name}-{fam}-{dt[0]}{D}", "steps", Sq, Sk, Hq, Hkv, D, causal, dt, fam, par, k_splits=ks)
         for name, par, Sq, Sk, causal, ks in [
             ("rise7.5", ("rise", 7.5), 192, 384, False, 0), ("rise8.5", ("rise", 8.5), 384, 384, True, 0),
             ("rise40", ("rise", 40.0), 192, 512, False, 0), ("rise8.5-ks2", ("rise", 8.5), 64, 512, False, 2),
             ("rise40-ks3", ("rise", 40.0), 192, 384, False, 3), ("fall", ("fall", 12.0, 30.0), 192, 384, False, 0),
             ("fall-ks3", ("fall", 12.0, 30.0), 384, 384, True, 3)]
         for fam, dt, D, Hq, Hkv in [("row64", _B, 128, 2, 1), ("row64", _F, 128, 4, 2), ("wave32", _F, 64, 2, 1),
                                     ("wave32", _B, 128, 4, 2)]]
# one ring step (merge_in, partial final rows) and two packed sequences on offset inputs: the shapes of
# tests/test_gpu_range.py::test_ring_step_with_a_running_lse_of_50_nat and ::test_offset_packed_on_the_32_row_family
RING = Case("offset-ring", "offset", 384, 384, 4, 2, 128, False, _B, None, (24.0, 1, 0.1, DO_MUL, DO_MEAN), seed=2)
PACKED = Case("offset-packed", "offset", 384, 384, 4, 2, 128, True, _B, "wave32", (24.0, 1, 0.1, DO_MUL, DO_MEAN), seed=3)
PACKED_SEQS = ((0, 250), (250, 134))                      # (first row, rows): the second starts on no tile boundary
EDGE = [Case(f"edge-{s}-{'bigk' if big else 'tame'}", "edge", 384, 192, 4, 2, 128, True, _F, None, (big,), scale=s)
        for s in (5.5, 5.6) for big in (False, True)]
ALL = OFFSET + SCALED + STEPS + EDGE + [RING]
BY_ID = {c.id: c for c in ALL}
assert len(BY_ID) == len(ALL)
