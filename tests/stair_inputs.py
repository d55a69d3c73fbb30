"""Seeded draws for the ragged sweeps of the document mask and the attention sinks (tests/test_gpu_fuzz_sink_doc.py, shown able
to fail by tests/test_fuzz_inputs_cpu.py): the (row_lo, key_hi) arrays of one launch, the needle edges that make one step of such
an array an O(1) error, and every single-step change of it.  Host arithmetic (numpy); nothing here loads the library.

A launch's mask is what include/usp_hip.h ("Document mask") admits: row i sees key j iff j >= row_lo[i] (and j <= i + Sk - Sq under
causal), row_lo non-decreasing with values in [0, Sk], key_hi its transpose.  Two generators:

  draw_doc_launch   lists of cumulative document lengths, cut into a launch by the library's own planner (ring/doc_blocks.py): the
                    whole sequence (Sq == Sk, causal) or the block of a ring below the diagonal (rows [row0, row0 + Sq) against the
                    earlier keys [key0, key0 + Sk), full).  Below the diagonal every row that sees a key belongs to the ONE
                    document that spans the gap, so such a block has at most two values of row_lo: its bound and Sk;
  draw_stair_launch staircases of up to 8 plateaus, which is what the ABI admits beyond documents.

Both return a namespace: kind ("whole" | "block" | "stairs"), B, Sq, Sk, causal, shared (one array for the batch: (n,) arrays, batch
stride 0), row_lo ((Sq,) or (B, Sq) int32), key_hi ((Sk,) or (B, Sk)), empty (per array: no row sees a key); the list launches also
lists, row0, key0.  Every extra draw of a case comes after the shape's (tests/test_gpu_fuzz.py: _dense_case).
"""
from types import SimpleNamespace

import numpy as np

PALETTE = (-30.0, 0.0, 3.0, 12.0, 1.5, -2.0, 6.0, 0.5)       # tests/test_gpu_sink.py::test_sink_grad_alone


def _near(rs, lo, hi, step):
    """An integer in [lo, hi]: half the time a multiple of `step`, or one before or one after it; otherwise uniform."""
    if rs.rand() < 0.5:
        x = step * int(rs.randint(lo // step, hi // step + 2)) + int(rs.choice([-1, 0, 1]))
    else:
        x = int(rs.randint(lo, hi + 1))
    return int(min(max(x, lo), hi))


def key_hi_of(row_lo, Sk):
    """The transpose of a non-decreasing row_lo: key_hi[j] = #{i : row_lo[i] <= j}."""
    return np.searchsorted(np.asarray(row_lo), np.arange(Sk, dtype=np.int64), side="right").astype(np.int32)


def plateaus(row_lo):
    """[(r0, r1, L)]: the maximal runs of rows [r0, r1) with one bound L."""
    rl = np.asarray(row_lo)
    cut = [0] + [int(i) + 1 for i in np.nonzero(np.diff(rl))[0]] + [len(rl)]
    return [(a, b, int(rl[a])) for a, b in zip(cut[:-1], cut[1:])]


# ---------------------------------------------------------------------------------------------------------------------
# document lists
# ---------------------------------------------------------------------------------------------------------------------
def draw_cu(rs, S, n_max=8):
    """One list [0, ..., S]: up to n_max boundaries, about half of them on / beside a multiple of 64, and in three cases of ten
    a run of six documents of length 1."""
    cut = set()
    if S >= 2:
        for _ in range(int(rs.randint(1, n_max + 1))):
            cut.add(_near(rs, 1, S - 1, 64))
        if S > 20 and rs.rand() < 0.3:
            s0 = int(rs.randint(1, S - 12))
            cut |= set(range(s0, s0 + 7))
    return [0] + sorted(cut) + [S]


def _block_list(rs, Sq, Sk, row0, key0, S_total, empty):
    """One list for the block of a ring below the diagonal.  Seeing: the document that spans the gap starts at key s_rel of the
    block (drawn on / beside the 64-key tiles) and ends behind row e_rel (on / beside the 32-row waves; Sq: behind the block);
    further boundaries lie in front of it and behind it, where they change nothing for this launch.  `empty`: a document starts
    in the gap or with the block's first row, so no row sees a key."""
    cut = set()
    if empty:
        cut.add(int(rs.randint(key0 + Sk, row0 + 1)))
    else:
        s = key0 + _near(rs, 0 if key0 > 0 else 1, Sk - 1, 64)      # (never position 0: a boundary that can move)
        e = row0 + _near(rs, 1, Sq, 32)
        cut |= {s, e}
        for _ in range(int(rs.randint(0, 3))):
            if s > 1:
                cut.add(int(rs.randint(1, s)))
    for _ in range(int(rs.randint(0, 3))):
        cut.add(int(rs.randint(max(cut) if cut else 1, S_total + 1)))
    return [0] + sorted(c for c in cut if 0 < c < S_total) + [S_total]


def launch_arrays(lists, row0, Sq, key0, Sk):
    """(row_lo, key_hi, empty) stacked over the lists, an entry that sees nothing as the planner fills it."""
    from yunchang_amd.ring import doc_blocks
    per = [doc_blocks.block_arrays(cu, row0, Sq, key0, Sk) for cu in lists]
    empty = [p is None for p in per]
    per = [doc_blocks.empty_arrays(Sq, Sk) if p is None else p for p in per]
    return np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), empty


def draw_doc_launch(rs, B, Sq, Sk):
    """A launch cut out of document lists.  Half the launches are the whole sequence (then Sk := Sq, causal), the others a block
    below the diagonal (full, Sq != Sk as drawn).  One list shared by the batch or B lists; with B lists a block holds, in six
    cases of ten, one entry that sees nothing beside the ones that do."""
    whole = bool(rs.rand() < 0.5) and Sq >= 2                   # (one position holds no boundary)
    shared = B == 1 or bool(rs.rand() < 0.3)
    n = 1 if shared else B
    if whole:
        Sk, row0, key0 = Sq, 0, 0
        lists = [draw_cu(rs, Sq, 8 if n == 1 else 4) for _ in range(n)]
    else:
        key0 = int(rs.choice([0, 64, rs.randint(1, 200)]))
        if Sk == 1:
            key0 = max(key0, 1)
        row0 = key0 + Sk + int(rs.choice([0, 0, rs.randint(1, 100)]))
        gone = int(rs.randint(n)) if (n > 1 and rs.rand() < 0.6) else -1
        lists = [_block_list(rs, Sq, Sk, row0, key0, row0 + Sq, i == gone) for i in range(n)]
    rl, kh, empty = launch_arrays(lists, row0, Sq, key0, Sk)
    assert not all(empty)
    if shared:
        rl, kh = rl[0], kh[0]
    return SimpleNamespace(kind="whole" if whole else "block", B=B, Sq=Sq, Sk=Sk, causal=whole, shared=shared, row_lo=rl,
                           key_hi=kh, empty=empty, lists=lists, row0=row0, key0=key0)


def list_mutants(launch):
    """Every boundary of every list moved by one position in each direction (onto its neighbour: the two documents merge), cut
    into the launch again -> ([(name, entry, row_lo of that entry)], number that leave the launch's mask as it was)."""
    from yunchang_amd.ring import doc_blocks
    out, same = [], 0
    for b, cu in enumerate(launch.lists):
        true = launch.row_lo if launch.shared else launch.row_lo[b]
        for i in range(1, len(cu) - 1):
            for move in (-1, 1):
                e = cu[i]
                mut = [x for x in cu if x != e] if not (cu[i - 1] < e + move < cu[i + 1]) else [e + move if x == e else x for x in cu]
                arr = doc_blocks.block_arrays(mut, launch.row0, launch.Sq, launch.key0, launch.Sk)
                rl = doc_blocks.empty_arrays(launch.Sq, launch.Sk)[0] if arr is None else arr[0]
                if _same_mask(rl, true, launch.Sq, launch.Sk, launch.causal):
                    same += 1
                else:
                    out.append((f"list {b} boundary {e} {move:+d}", b, rl))
    return out, same


# ---------------------------------------------------------------------------------------------------------------------
# staircases
# ---------------------------------------------------------------------------------------------------------------------
def draw_staircase(rs, Sq, Sk, causal):
    """(row_lo, key_hi): up to 8 plateaus.  Half the plateau edges sit on / beside a multiple of 32 (the wave height), half the
    bounds on / beside a multiple of 64 (the key tile); 0 opens the staircase in half the cases and Sk closes it in three of ten.
    Under `causal` a plateau that opens at row r0 draws its bound, in 85 cases of 100, from the keys row r0 sees with one to
    spare (<= r0 + Sk - Sq - 1): most rows then see at least two keys, and one step of the array changes the mask (uniform bounds
    mostly hide every key of the rows they cover, where a step changes nothing).  The two arrays are asserted to describe one
    mask (tests/doc_ref.py: block_mask, mask_of_key_hi)."""
    import doc_ref
    import torch
    n = int(rs.randint(1, 9))
    edges = sorted({_near(rs, 1, Sq - 1, 32) for _ in range(n - 1)}) if Sq >= 2 else []
    b = [0] + edges + [Sq]
    rl = np.zeros(Sq, dtype=np.int32)
    lo = 0
    for p, (r0, r1) in enumerate(zip(b[:-1], b[1:])):
        last = p == len(b) - 2
        if p == 0 and rs.rand() < 0.5:
            val = 0
        elif last and len(b) > 2 and rs.rand() < 0.3:
            val = Sk
        else:
            hi = Sk
            if causal and rs.rand() < 0.85:
                hi = min(Sk, max(lo, r0 + Sk - Sq - 1))
            val = _near(rs, lo, hi, 64)
        rl[r0:r1] = val
        lo = val
    kh = key_hi_of(rl, Sk)
    assert (np.diff(rl) >= 0).all() and rl.min() >= 0 and rl.max() <= Sk and (np.diff(kh) >= 0).all()
    assert torch.equal(doc_ref.block_mask(rl, Sq, Sk, causal), doc_ref.mask_of_key_hi(kh, Sq, Sk, causal)), "row_lo / key_hi disagree"
    return rl, kh


def draw_stair_launch(rs, B, Sq, Sk, causal):
    """A launch of staircases: one for the batch or one per entry."""
    shared = B == 1 or bool(rs.rand() < 0.3)
    per = [draw_staircase(rs, Sq, Sk, causal) for _ in range(1 if shared else B)]
    rl, kh = np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
    empty = [not _visible(r, Sq, Sk, causal).any() for r in rl]
    if shared:
        rl, kh = rl[0], kh[0]
    return SimpleNamespace(kind="stairs", B=B, Sq=Sq, Sk=Sk, causal=causal, shared=shared, row_lo=rl, key_hi=kh, empty=empty)


def _visible(row_lo, Sq, Sk, causal):
    """(Sq, Sk) bool, numpy: tests/doc_ref.py's block_mask."""
    j = np.arange(Sk)[None, :]
    m = j >= np.asarray(row_lo, dtype=np.int64)[:, None]
    return m & (j <= np.arange(Sq)[:, None] + (Sk - Sq)) if causal else m


def _same_mask(a, b, Sq, Sk, causal):
    return bool((_visible(a, Sq, Sk, causal) == _visible(b, Sq, Sk, causal)).all())


def stair_edges(row_lo, Sq, Sk, causal):
    """(row, key) pairs for tests/needle_inputs.py: make(..., edges=...) under which ONE step of `row_lo` is an O(1) error; it
    generalises tests/doc_ref.py: needle_edges to any staircase.  For every plateau with bound L over rows [r0, r1):
      - key L - 1, the last hidden key, for rows r0 and r0 + 1: wrongly seen, it takes its share of the row's mass;
      - keys L and L + 1 for rows r0, r0 + 1, r1 - 2 and r1 - 1 where the row's right bound lets it see them: wrongly hidden, L
        takes its share with it, and L + 1 keeps a second key in the row (a row whose mass sits on one key has dS = 0 whatever
        it sees);
      - the bound L' of the plateau in front and L' + 1, where they lie below L, for rows r0 - 1 and r0: the edge between the
        plateaus moved by one row shows or hides them."""
    end = lambda r: min(Sk - 1, r + Sk - Sq) if causal else Sk - 1
    out, prev = [], None
    for r0, r1, L in plateaus(row_lo):
        if L > 0:
            out += [(r, L - 1) for r in (r0, r0 + 1) if r < r1]
        for r in (r0, r0 + 1, r1 - 2, r1 - 1):
            if r0 <= r < r1:
                out += [(r, j) for j in (L, L + 1) if j <= end(r)]
        if prev is not None:
            out += [(r, j) for r in (r0 - 1, r0) for j in (prev, prev + 1) if j < L and j <= end(r)]
        prev = L
    return sorted(set(out))


def launch_edges(launch):
    """stair_edges of every array of a launch, in one list (the inputs are shared by the batch)."""
    rl = np.asarray(launch.row_lo).reshape(-1, launch.Sq)
    return sorted(set(e for r in rl for e in stair_edges(r, launch.Sq, launch.Sk, launch.causal)))


def mutants(row_lo, Sq, Sk, causal):
    """Every single-step change of a staircase -> ([(name, row_lo)], number dropped because the mask stays as it was): one
    plateau's bound moved by one key in each direction (inside [0, Sk]), one plateau edge moved by one row in each direction."""
    rl = np.asarray(row_lo)
    out, same = [], 0
    cand = []
    ps = plateaus(rl)
    for p, (r0, r1, L) in enumerate(ps):
        for move in (-1, 1):
            m = rl.copy()
            m[r0:r1] = min(max(L + move, 0), Sk)
            cand.append((f"rows [{r0}, {r1}) bound {L} {move:+d}", m))
        if p > 0:
            m = rl.copy()
            m[r0 - 1] = L
            cand.append((f"edge at row {r0} one row up", m))
            m = rl.copy()
            m[r0] = ps[p - 1][2]
            cand.append((f"edge at row {r0} one row down", m))
    for name, m in cand:
        if _same_mask(m, rl, Sq, Sk, causal):
            same += 1
        else:
            out.append((name, m))
    return out, same


def launch_mutants(launch):
    """The single-step changes of a launch, one array at a time -> ([(name, entry, row_lo of that entry)], number dropped):
    list_mutants for a launch cut out of lists, mutants for staircases."""
    if launch.kind != "stairs":
        return list_mutants(launch)
    out, same = [], 0
    for b, rl in enumerate(np.asarray(launch.row_lo).reshape(-1, launch.Sq)):
        got, s = mutants(rl, launch.Sq, launch.Sk, launch.causal)
        out += [(f"array {b} {name}", b, m) for name, m in got]
        same += s
    return out, same


# ---------------------------------------------------------------------------------------------------------------------
# sinks
# ---------------------------------------------------------------------------------------------------------------------
def draw_sinks(rs, Hq):
    """(Hq,) fp32 from PALETTE; one head is forced to 12 (a sink above every score) and, with more than one head, its neighbour
    to -30 or 0 (no effect, off-by-one softmax): sinks read for the wrong head are an O(1) error."""
    s = np.array([PALETTE[i] for i in rs.randint(0, len(PALETTE), size=Hq)], dtype=np.float32)
    h = int(rs.randint(Hq))
    s[h] = 12.0
    if Hq > 1:
        s[(h + 1) % Hq] = float(rs.choice([-30.0, 0.0]))
    return s
