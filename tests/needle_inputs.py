"""Structured "needle" inputs: q, k, v, dout on which a lost, doubled or mispaired key tile is an O(1) error.

N(0,1) inputs with softmax_scale = D^-0.5 make attention a near-uniform average over the visible keys: a row that sees N
keys has an output of standard deviation ~sqrt(e / N), and one 64-key tile carries 64 / N of its mass -- below the stated
absolute tolerance from a few thousand keys on (tests/test_needle_cpu.py pins that).  Here the softmax mass of every row
sits on a handful of sparse needle keys placed by the kernels' own structure:

- C class directions: rows 1..C of the Sylvester +-1 Hadamard matrix of size D (C <= D - 1, mutually orthogonal);
- query (row i, head h) has class `q_class(i, h)` = (i + phase(h)) mod C and q = a * h_c + Q_NOISE * noise, with
  a = 1.25 * sqrt(128 / D): a needle of the row's class scores a * D * D^-0.5 = 14.1 nat at every D;
- the query heads of one KV group have different phases (a wrong head inside a group, or a wrong group, attends other
  needles: an O(1) error);
- background keys are BG * noise (scores ~0); every 64-key tile t (kBN = kTile = 64) of KV head hk holds ONE needle of
  class (t + 5 hk) mod C, k = h_c + K_NOISE * noise', at an offset that varies from tile to tile: 0 in tiles t = 0 mod 8,
  63 in tiles t = 7 mod 8, random between (the nearest key beside it where an edge needle sits there);
- the noise of needles and queries is orthogonal to every direction in use: the needles of one
  class differ in direction (dS sums to zero along a row, so parallel needle keys would leave dQ blind) while their
  scores differ only through the q-noise x k-noise term, std <= Q_NOISE * K_NOISE = 0.3 nat: the weights spread without
  ever saturating;
- the query noise makes the elements of a needle's dK row differ in size and sign, so that the contribution of a few rows
  is not hidden behind rtol * |dK| of a sum over hundreds of rows;
- v is N(0,1); dout is N(0,1) on the rows named in `edges` and DO_MUL x N(0,1) on all others.  (At full amplitude the
  honest 16-bit rounding of P and dS already costs up to 1.6x the stated dK / dV tolerance on these inputs -- P is O(1)
  here, hundreds of rows attend one needle key, and the error of such a sum is absolute, not relative to each element:
  measured on the kernels and reproduced to three digits by the rounding model of tests/test_needle_cpu.py, SURVEY.md
  section 8(c).  The amplitude is lowered until that model keeps a 2x margin; the edge rows, few, keep theirs.)
- every class occurs in every C consecutive rows, hence in every 256-row tile and (C <= 64) in every 128-row tile and
  64-row wave: every visible (query tile, key tile) pair is needed by some row;
- `edges`: (row, key) pairs.  Every row named there gets, in one head of each KV group, a second, PRIVATE direction
  (Hadamard rows C+1.., shared only by rows 64 named rows apart) on top of its class, and key `key` becomes a needle of
  that private direction (of the sum of them when several rows name one key): it weighs as much as a class needle for that row and nothing for any other, so its dK / dV row
  is the contribution of that one row -- losing or doubling one (row, key) pair is a 100 % error there, not one of a
  hundred terms.  The helpers below list the pairs of a case's mask edges (last visible and first invisible key) and of
  the boundaries of key runs, key blocks and query runs.

Everything is rounded to the 16-bit dtype at the end: the values are exactly representable, the fp64 reference and the
kernels read the same numbers.  |score * log2(e)| stays below 24 (needles ~20.4), K * scale * log2(e) below 1: inside the
exponent range of both 16-bit types.  (Values outside this envelope, and scales other than D^-0.5: tests/range_inputs.py.)
"""
from types import SimpleNamespace

import numpy as np

from golden_util import round_to

TILE = 64
Q_AMP, Q_NOISE, K_NOISE, BG = 1.25, 0.5, 0.6, 0.25
DO_MUL = 0.25


def do_mul_for(G):
    """The amplitude of dout on ordinary rows: the 16-bit rounding of P and dS leaves an ABSOLUTE error on a needle's dK /
    dV row that grows with the number of rows attending it (~sqrt(G) at equal depth); 0.25 (0.125 at G = 8) keeps the
    rounding model of tests/test_needle_cpu.py inside half of the stated tolerance."""
    return 0.125 if G >= 8 else DO_MUL


def hadamard(n):
    assert n & (n - 1) == 0, n
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def head_phase(h, G, C):
    return (h % G) * max(1, C // G) + h // G


def q_class(i, h, G, C):
    return (i + head_phase(h, G, C)) % C


def make(Sq, Sk, Hq, Hkv, D, dt, C, seed=0, B=1, edges=(), segments=None, q_mul=1.0, do_mul=None):
    """-> namespace(q (B,Sq,Hq,D), k, v (B,Sk,Hkv,D), do: float32 arrays of values exact in `dt`; needle (Sk,Hkv) bool;
    kdir (Sk,Hkv,D): the sum of the directions a needle key carries (0: background); qdir (Sq,Hq,D): the directions of a
    query (class + private)).  `segments`: (first key, keys) of every packed sequence (the 64-key tiles of a packed
    sequence start at its first key); default one segment [0, Sk).  `q_mul`: a power of two on q (needle scores 14.1 * q_mul nat: for a softcap that bites)."""
    assert 1 <= C <= D - 2 and Hq % Hkv == 0
    G = Hq // Hkv
    E = min((D - C) // 2, 64)                                        # private directions of the edge needles
    rs = np.random.RandomState(1000 + seed)
    H = hadamard(D)[1:C + E + 1]                                     # (C + E, D)
    qcls = (np.arange(Sq)[:, None] + np.array([head_phase(h, G, C) for h in range(Hq)])[None, :]) % C
    owners = {}                                                      # (key, kv head) -> directions of the needle there
    edge_keys = {key for row, key in edges if 0 <= key < Sk and 0 <= row < Sq}
    for first, n in (segments or [(0, Sk)]):
        for t in range(-(-n // TILE)):
            for hk in range(Hkv):
                off = 0 if t % 8 == 0 else (TILE - 1 if t % 8 == 7 else int(rs.randint(1, TILE - 1)))
                pos = first + min(t * TILE + off, n - 1)
                lo, hi = first + t * TILE, first + min((t + 1) * TILE, n)
                free = sorted((j for j in range(lo, hi) if j not in edge_keys), key=lambda j: abs(j - pos))
                if free:                                             # (beside an edge needle, never on it: no key may
                    owners[(free[0], hk)] = [(t + 5 * hk) % C]       # score twice for one row)
    qdir = H[qcls].copy()                                            # (Sq, Hq, D)
    pdir = np.zeros_like(qdir)                                       # the private part of it
    ids = {}
    for row, key in edges:
        if not (0 <= key < Sk and 0 <= row < Sq):
            continue
        if row not in ids:
            ids[row] = len(ids)
            for hk in range(Hkv):
                pdir[row, hk * G + ids[row] % G] = H[C + ids[row] % E]
        for hk in range(Hkv):
            own = owners.setdefault((key, hk), [])
            if C + ids[row] % E not in own:
                own.append(C + ids[row] % E)
    a = Q_AMP * (128.0 / D) ** 0.5
    nq = Q_NOISE * rs.standard_normal((B, Sq, Hq, D))                # orthogonal to every direction in use: a query's
    nq -= (nq @ H.T) @ H / D                                         # needles score alike, however many rows share a key
    qdir += pdir
    q = (a * qdir[None] + nq) * q_mul
    k = BG * rs.standard_normal((B, Sk, Hkv, D))
    kdir = np.zeros((Sk, Hkv, D))
    for (key, hk), own in owners.items():
        for o in own:
            kdir[key, hk] += H[o]
    needle = np.abs(kdir).sum(-1) > 0
    for hk in range(Hkv):                                            # no key carries two directions of one query
        twice = qdir[:, hk * G:(hk + 1) * G].reshape(-1, D) @ kdir[needle[:, hk], hk].T > 1.5 * D
        assert not twice.any(), "a needle key carries two directions of one query"
    nz = K_NOISE * rs.standard_normal((B, int(needle.sum()), D))     # orthogonal to EVERY direction in use: a needle's
    nz -= (nz @ H.T) @ H / D                                         # noise moves no query's score but through q's noise
    k[:, needle] = kdir[needle][None] + nz
    v = rs.standard_normal((B, Sk, Hkv, D))
    do = rs.standard_normal((B, Sq, Hq, D))
    amp = np.full(Sq, do_mul_for(G) if do_mul is None else do_mul)          # (the rows named in `edges` keep dout at N(0,1))
    amp[list(ids)] = 1.0
    do *= amp[None, :, None, None]
    q, k, v, do = (round_to(x.astype(np.float32), dt) for x in (q, k, v, do))
    return SimpleNamespace(q=q, k=k, v=v, do=do, needle=needle, kdir=kdir, qdir=qdir, C=C)


# ---------------------------------------------------------------------------------------------------------------------
# where the edge needles go
# ---------------------------------------------------------------------------------------------------------------------
def sample_rows(Sq, n=24, seed=0):
    """Rows at tile, wave and sequence edges plus a seeded draw."""
    rs = np.random.RandomState(77 + seed)
    fixed = [0, 1, 63, 64, 127, 128, 255, 256, Sq // 2 - 1, Sq // 2, Sq - 257, Sq - 256, Sq - 65, Sq - 64, Sq - 2, Sq - 1]
    rows = set(r for r in fixed if 0 <= r < Sq) | set(int(r) for r in rs.randint(0, Sq, size=n))
    return sorted(rows)


def _bounds(Sq, Sk, causal, window, shift=0):
    """(left, right, off) of a mask as include/usp_hip.h defines it: row i sees key j iff i + off - left <= j <= i + off + right
    (each side only where its bound is >= 0), off = Sk - Sq + shift; `causal` sets right = 0.  A shift with neither `causal`
    nor a window is ignored (there is no bound it could move)."""
    left, right = (-1, -1) if window is None else (int(window[0]), int(window[1]))
    if causal:
        right = 0
    return left, right, Sk - Sq + (int(shift or 0) if (left >= 0 or right >= 0) else 0)


def mask_edges(rows, Sq, Sk, causal=False, window=None, shift=0):
    """(row, key) pairs: the last visible and the first invisible key of each row on every bound of its mask (the causal
    diagonal with its Sk - Sq + shift offset, the window's left and right bound)."""
    left, right, off = _bounds(Sq, Sk, causal, window, shift)
    out = []
    for r in rows:
        if right >= 0:
            out += [(r, r + off + right), (r, r + off + right + 1)]
        if left >= 0:
            out += [(r, r + off - left), (r, r + off - left - 1)]
    return [(r, j) for r, j in out if 0 <= j < Sk]


def _visible(r, j, Sq, Sk, causal, window, shift=0):
    left, right, off = _bounds(Sq, Sk, causal, window, shift)
    d = j - (r + off)
    return (right < 0 or d <= right) and (left < 0 or d >= -left)


def key_tiles_of_query_tile(q0, rows, Sq, Sk, causal, window=None, shift=0):
    """[t0, nt): the 64-key tiles a query tile [q0, q0 + rows) streams (usp_flash_fwd_body.inc, usp_flash_fwd64.hip).  With a
    `shift` the causal limit and the left bound move with the diagonal; a right window bound without `causal` limits the range
    as the causal limit does (the causal instantiation serves it, with causal_off = Sk - Sq + shift + right)."""
    left, right, off = _bounds(Sq, Sk, causal, window, shift)
    e = Sk
    if right >= 0:
        e = min(e, min(q0 + rows, Sq) + off + right)
    nt = -(-e // TILE) if e > 0 else 0
    t0 = 0
    if left >= 0:
        t0 = min(nt, max(0, q0 + off - left) // TILE)
    return t0, nt


def run_bounds(t0, nt, n, rule):
    """Tile indices where the runs of a cut of tiles [t0, nt) into n begin: rule "floor" = the forward K split
    (t0 + s * (nt - t0) // n), rule "per" = the backward cuts (equal runs of ceil((nt - t0) / n) tiles)."""
    if n <= 1:
        return []
    if rule == "floor":
        b = [t0 + s * (nt - t0) // n for s in range(1, n)]
    else:
        per = -(-(nt - t0) // n)
        b = [min(nt, t0 + s * per) for s in range(1, n)]
    return sorted(set(x for x in b if t0 < x < nt))


def _spread(rows, salt, n):
    """n entries of `rows` spread over the list, another choice for another `salt`."""
    if not rows:
        return []
    return sorted(set(rows[(salt + i * max(1, len(rows) // n)) % len(rows)] for i in range(n)))


def key_run_edges(Sq, Sk, causal, n, rule, window=None, tile_rows=256, per=3, tiles=None, shift=0):
    """(row, key) pairs for the first and the last key of every run of a key cut into n (forward `k_splits`: rule "floor";
    `dq_splits`: rule "per"), for every query tile: 2 * `per` rows of the tile that see both keys get a needle on one of them, in turn.  `tiles`: first rows of
    the query tiles to do this for (default: all; every named row sees the needles of the rows that share its private
    direction, so name few in one launch)."""
    out = []
    for q0 in (range(0, Sq, tile_rows) if tiles is None else tiles):
        t0, nt = key_tiles_of_query_tile(q0, tile_rows, Sq, Sk, causal, window, shift)
        for tb in run_bounds(t0, nt, n, rule):
            kb = tb * TILE
            rows = [r for r in range(q0, min(q0 + tile_rows, Sq)) if kb < Sk and
                    _visible(r, kb, Sq, Sk, causal, window, shift) and _visible(r, kb - 1, Sq, Sk, causal, window, shift)]
            for i, r in enumerate(_spread(rows, 7 * tb + q0 // tile_rows + (11 if rule == "per" else 0), 2 * per)):
                out.append((r, kb - 1 + i % 2))              # (one key per row: few needles per row keep P large)
    return out


def key_block_edges(Sq, Sk, causal, window=None, block=128, every=1, per=3, shift=0):
    """(row, key) pairs on the last key of a 128-key dK/dV block and the first of the next (every `every`-th boundary),
    each for `per` rows among the last 256 of the launch that see the pair."""
    out = []
    for kb in range(block, Sk, block * every):
        rows = [r for r in range(max(0, Sq - 256), Sq)
                if _visible(r, kb, Sq, Sk, causal, window, shift) and _visible(r, kb - 1, Sq, Sk, causal, window, shift)]
        for i, r in enumerate(_spread(rows, 5 * (kb // block), 2 * per)):
            out.append((r, kb - 1 + i % 2))
    return out


def query_run_edges(Sq, Sk, causal, n, block=128, every=1, per=3, shift=0):
    """(row, key) pairs for a dK/dV cut into n (`dkdv_splits`): for (every `every`-th) 128-key block, the last and the
    first query row of adjacent runs (usp_flash_bwd64.hip: 64-row query tiles [t_begin, t_end) in equal runs) each get
    `per` needles inside the block -- the rows whose contribution a wrong run boundary loses or doubles."""
    out = []
    nq = -(-Sq // TILE)
    for kb in range(0, Sk, block * every):
        t_begin = max(0, kb - (Sk - Sq + int(shift or 0))) // TILE if causal else 0
        for t in run_bounds(min(t_begin, nq), nq, n, "per"):
            for i, r in enumerate((t * TILE - 1, t * TILE)):
                keys = [j for j in range(kb, min(kb + block, Sk)) if 0 <= r < Sq and _visible(r, j, Sq, Sk, causal, None, shift)]
                out += [(r, j) for j in _spread(keys, 29 * (2 * t + i) + 3, per)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# conditions on the inputs (asserted from the fp64 reference: not tolerances)
# ---------------------------------------------------------------------------------------------------------------------
def needle_stats(nd, rows, scale, visible, b=0, softcap=None):
    """For each sampled row and every head: (needles of its directions it sees, needle mass, largest single weight).
    `visible(r)` -> bool (Sk,) mask of row r.  fp64 numpy."""
    Hq, Hkv = nd.q.shape[2], nd.k.shape[2]
    G = Hq // Hkv
    k64 = nd.k[b].astype(np.float64)
    D = nd.q.shape[-1]
    res = []
    for r in rows:
        vis = visible(r)
        if not vis.any():
            continue
        for h in range(Hq):
            s = k64[:, h // G] @ nd.q[b, r, h].astype(np.float64) * scale
            if softcap:
                s = softcap * np.tanh(s / softcap)
            s = np.where(vis, s, -np.inf)
            p = np.exp(s - s.max())
            p /= p.sum()
            own = vis & (nd.kdir[:, h // G] @ nd.qdir[r, h] > 0.5 * D)
            res.append((int(own.sum()), float(p[own].sum()), float(p.max())))
    return res


def assert_needle_conditions(nd, rows, scale, visible, what="", softcap=None):
    """Needle mass >= 0.98 for every sampled row that sees a needle of its class; largest single weight <= 0.9 for rows
    that see at least two."""
    st = needle_stats(nd, rows, scale, visible, softcap=softcap)
    seen = [s for s in st if s[0] >= 1]
    assert seen, what + ": no sampled row sees a needle of its class"
    mass = min(s[1] for s in seen)
    assert mass >= 0.98, f"{what}: needle mass {mass:.4f} < 0.98"
    two = [s[2] for s in st if s[0] >= 2]
    if two:
        assert max(two) <= 0.9, f"{what}: largest single weight {max(two):.4f} > 0.9 on a row with >= 2 needles"
    return mass, (max(two) if two else None), len(seen)


# ---------------------------------------------------------------------------------------------------------------------
# the verdict: the suite's comparator and stated tolerances, with the worst error / bound of every tensor
# ---------------------------------------------------------------------------------------------------------------------
def bound_ratio(got, want, atol, rtol):
    """(all elements pass golden_util.close_mask, max over elements of err / (atol + rtol |want|)); a NaN or a wrong
    infinity counts as an infinite ratio.  numpy arrays or torch tensors (then computed on the device)."""
    from golden_util import close_mask
    ok, err = close_mask(got, want, atol, rtol)
    if isinstance(ok, np.ndarray):
        w = np.abs(np.asarray(want, dtype=np.float64))
        lim = atol + rtol * np.where(np.isfinite(w), w, 0.0)
        ratio = np.where(ok, np.where(np.isfinite(err), err, 0.0) / lim, np.where(np.isfinite(err), err / lim, np.inf))
        return bool(ok.all()), float(ratio.max()) if ratio.size else 0.0
    import torch
    if ok.numel() == 0:
        return True, 0.0
    w = want.detach().to(device=ok.device, dtype=torch.float64).abs() if isinstance(want, torch.Tensor) else \
        torch.from_numpy(np.abs(np.asarray(want, dtype=np.float64))).to(ok.device)
    lim = atol + rtol * torch.where(torch.isfinite(w), w, torch.zeros_like(w))
    fin = torch.isfinite(err)
    ratio = torch.where(fin, err / lim, torch.where(ok, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return bool(ok.all()), float(ratio.max())


def verdicts(got, want, dt, Sq, Sk, G):
    """{tensor: (passes, worst err / bound)} for the tensors present in `got` among out, lse, dq, dk, dv, judged as every
    GPU parity file judges them: golden_util.TOL, lse 2e-3 + 1e-4 |lse|, golden_util.long_sum_atol on gradient sums of
    >= 1000 products.  This is what tests/test_gpu_needle.py asserts and what tests/test_needle_cpu.py requires every
    mutant to fail."""
    from golden_util import TOL, long_sum_atol
    res = {}
    for n_ in ("out", "lse", "dq", "dk", "dv"):
        if n_ not in got:
            continue
        if n_ == "out":
            atol, rtol = TOL[dt]["out"]
        elif n_ == "lse":
            atol, rtol = 2e-3, 1e-4
        else:
            atol, rtol = TOL[dt]["grad"]
            atol = long_sum_atol(atol, Sk if n_ == "dq" else Sq * G, want[n_])
        res[n_] = bound_ratio(got[n_], want[n_], atol, rtol)
    return res
