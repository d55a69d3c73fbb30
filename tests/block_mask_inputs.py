"""Case tables and mask makers of the block-sparse edge tests (tests/test_gpu_block_mask_edges.py on the GPU,
tests/test_block_mask_inputs_cpu.py without one).  Nothing of the package is imported: masks are numpy bool arrays, the lists come
from block_mask_ref.enumerate_lists, needle inputs from tests/needle_inputs.py.

RAGGED   sequence ends: S in {64, 257, 300, 320, 449} -- one block of one tile; a last tile of one key with no second tile; a last
         tile of 44 keys; a full last tile with the second absent; a second tile of one key -- over three head shapes, B in {1, 2},
         both dtypes, causal and full, four masks.  White noise.
LONG     lists past 64 and 128 entries: S = 4400 (35 blocks, 69 tiles, the last block one tile of 48 keys) and S = 8300 (65 blocks,
         130 tiles); `dense` masks at 0.97 per head and circulant masks whose lists hold 61 ... 68 entries.  Needle inputs with edge
         needles at the list positions 0, 63, 64, 65 and last.
HEADS    the dK/dV head walk: per (b, key block) slot of a KV group a stated set of query heads whose transposed list is empty.
fuzz_case  one seeded case of the sweep.
"""
from types import SimpleNamespace

import numpy as np
import torch

import block_mask_ref as R
import needle_inputs as NI

BLOCK, TILE = 128, 64
SHAPES3 = [(3, 1, 32), (4, 2, 128), (2, 2, 64)]                     # (Hq, Hkv, D)
DTYPES = ("bfloat16", "float16")


def m4_of(mask, B, Hq):
    """A 2-d, 3-d or 4-d numpy mask broadcast to (B, Hq, nb, nb)."""
    m = np.asarray(mask)
    nb = m.shape[-1]
    return np.broadcast_to(m.reshape((1,) * (4 - m.ndim) + m.shape), (B, Hq, nb, nb))


# ------------------------------------------------------------------------------------------------------------------------------
# RAGGED
# ------------------------------------------------------------------------------------------------------------------------------
RAGGED_S = (64, 257, 300, 320, 449)
RAGGED_MASKS = ("all", "random", "last_only", "holes")


def one_tile_last_block(S):
    """The last 128-block has no second 64-tile: S mod 128 in (0, 64]."""
    return 0 < S % BLOCK <= TILE


def ragged_mask(kind, B, Hq, S, seed=0):
    nb = R.n_blocks(S)
    rs = np.random.RandomState(4000 + 13 * S + 7 * Hq + B + 100 * seed)
    if kind == "all":
        return np.ones((B, Hq, nb, nb), dtype=bool)
    if kind == "random":
        return rs.rand(B, Hq, nb, nb) < 0.5
    if kind == "last_only":              # only the last key-block column and the last row-block row are live
        m = np.zeros((B, Hq, nb, nb), dtype=bool)
        m[:, :, nb - 1, :] = True
        m[:, :, :, nb - 1] = True
        return m
    assert kind == "holes", kind         # as tests/test_gpu_block_mask.py: one row block and one key block all false
    m = rs.rand(B, Hq, nb, nb) < 0.6
    m[:, :, nb // 2, :] = False
    m[:, :, :, nb // 3] = False
    return m


def ragged_cases():
    out = []
    for i_s, S in enumerate(RAGGED_S):
        for i_b, B in enumerate((1, 2)):
            for i_d, dt in enumerate(DTYPES):
                for causal in (True, False):
                    for i_m, kind in enumerate(RAGGED_MASKS):
                        Hq, Hkv, D = SHAPES3[(i_s + i_b + i_d + i_m) % 3]
                        out.append(SimpleNamespace(S=S, B=B, Hq=Hq, Hkv=Hkv, D=D, dt=dt, causal=causal, kind=kind,
                                                   id=f"S{S}-B{B}-H{Hq}/{Hkv}-D{D}-{dt}-{'causal' if causal else 'full'}-{kind}"))
    return out


RAGGED = ragged_cases()


# ------------------------------------------------------------------------------------------------------------------------------
# LONG
# ------------------------------------------------------------------------------------------------------------------------------
LONG_SHAPES = [(4400, 4, 2, 128, "bfloat16"), (4400, 2, 2, 64, "float16"), (8300, 1, 1, 32, "bfloat16")]    # (S, Hq, Hkv, D, dt), B = 1
LONG_MASKS = [("dense", True), ("dense", False), ("circ31", False), ("circ32", False), ("circ33", False)]
POSITIONS = (0, 63, 64, 65)              # list positions that get an edge needle, beside the last one (and 128 where it exists)
ROW_OFFSETS = (0, 37, 64, 127)


def long_mask(kind, Hq, S, seed=0):
    """`dense`: (1, Hq, nb, nb) at 0.97 per head; the last two row blocks and the first two key blocks are all set, so that under
    causal too every family has lists of every block (66 entries and more at S = 4400, 129 and more at S = 8300).
    `circ<w>`: the 2-d mask[r, c] = ((c - r) mod nb) < w, the same for every head."""
    nb = R.n_blocks(S)
    if kind == "dense":
        m = np.random.RandomState(5000 + S + Hq + 100 * seed).rand(1, Hq, nb, nb) < 0.97
        m[:, :, nb - 2:, :] = True
        m[:, :, :, :2] = True
        return m
    w = int(kind[4:])
    r, c = np.arange(nb)[:, None], np.arange(nb)[None, :]
    return ((c - r) % nb) < w


def list_lengths(lists):
    """family -> sorted list of the lengths that occur."""
    return {fam: sorted(set(len(e) for e in d.values())) for fam, d in lists.items()}


def _positions(n):
    return sorted(set(p for p in POSITIONS + (128, n - 1) if 0 <= p < n))


def long_edges(m4, S, Hq, Hkv, causal, lists, seed=0):
    """Edge needles of a LONG case -> (edges for needle_inputs.make, records).  A seeded sample of row blocks (two whose forward
    lists hold >= 66 entries in every head -- the longest where none does --, and the last one): the rows at offsets 0, 37, 64 and 127 each name one key in the tiles
    at positions 0, 63, 64, 65 and last of their forward list.  Likewise for the transposed lists: the keys at those offsets of two
    sampled key blocks against rows in the row tiles at those positions.  A named row carries its private direction in head
    (order of naming) mod G of every KV group (needle_inputs.make), so the lists read are that head's, and a pair is taken only if
    that head sees it in every group.  records: (family, block, head, position, row, key)."""
    G, nb = Hq // Hkv, m4.shape[-1]
    rs = np.random.RandomState(6000 + seed + S)
    ids, edges, seen, records = {}, [], set(), []

    def head_of(row):
        return ids.get(row, len(ids)) % G

    def sees(row, key):
        h = head_of(row)
        return (not causal or key <= row) and all(m4[0, hk * G + h, row // BLOCK, key // BLOCK] for hk in range(Hkv))

    def add(fam, blk, pos, row, key):
        h = head_of(row)
        ids.setdefault(row, len(ids))
        if (row, key) not in seen:
            seen.add((row, key))
            edges.append((row, key))
        records.append((fam, blk, h, pos, row, key))

    def sample(fam):
        shortest = [min(len(lists[fam][0, h, x]) for h in range(Hq)) for x in range(nb)]
        need = min(66, sorted(shortest)[-2])               # (circ31 has no list of 66: its longest then)
        ok = [x for x in range(nb) if shortest[x] >= need]
        odd = [x for x in ok if x % 2] or ok                # one odd block: the second of a dQ pair, whose last key blocks close the pair's list
        first = int(rs.choice(odd))
        return sorted([first, int(rs.choice([x for x in ok if x != first]))])
    row_blocks = sorted(set(sample("fwd") + [nb - 1]))
    key_blocks = sample("dkdv")
    for r in row_blocks:
        for off in ROW_OFFSETS:
            row = BLOCK * r + off
            if row >= S:
                continue
            ent = lists["fwd"][0, head_of(row), r]
            for p in _positions(len(ent)):
                for o in rs.permutation(TILE):
                    key = ent[p] * TILE + int(o)
                    if key < S and (row, key) not in seen and sees(row, key):
                        add("fwd", r, p, row, key)
                        break
    for c in key_blocks:
        for off in ROW_OFFSETS:
            key = BLOCK * c + off
            if key >= S:
                continue
            n = len(lists["dkdv"][0, len(ids) % G, c])
            for p in _positions(n):
                ent = lists["dkdv"][0, len(ids) % G, c]        # the head a newly named row gets
                if p >= len(ent):
                    continue
                for o in rs.permutation(TILE):
                    row = ent[p] * TILE + int(o)
                    if row < S and row not in ids and sees(row, key):
                        add("dkdv", c, p, row, key)
                        break
    return edges, SimpleNamespace(records=records, row_blocks=row_blocks, key_blocks=key_blocks, ids=ids)


def long_cases():
    out = []
    for S, Hq, Hkv, D, dt in LONG_SHAPES:
        for kind, causal in LONG_MASKS:
            out.append(SimpleNamespace(S=S, B=1, Hq=Hq, Hkv=Hkv, D=D, dt=dt, causal=causal, kind=kind, G=Hq // Hkv,
                                       id=f"S{S}-H{Hq}/{Hkv}-D{D}-{dt}-{'causal' if causal else 'full'}-{kind}"))
    return out


LONG = long_cases()
_LONG_BUILT = {}


def long_build(c, white=False):
    """The mask (as handed to the kernels: 4-d for `dense`, 2-d for `circ`), its (1, Hq, nb, nb) expansion, the enumerated lists, the
    edge needles and the needle inputs of a LONG case; cached.  The table's own claims are asserted here: a `dense` case has a list
    of >= 65 entries in every family (>= 129 at S = 8300); the needle conditions hold under block_mask_ref.visible.
    `white`: N(0, 1) inputs in the case's dtype instead (the record of why needles are used)."""
    key = (c.id, white)
    if key in _LONG_BUILT:
        return _LONG_BUILT[key]
    mask = long_mask(c.kind, c.Hq, c.S)
    m4 = np.array(m4_of(mask, 1, c.Hq))
    lists = R.enumerate_lists(m4, c.S, c.causal)
    lens = list_lengths(lists)
    if c.kind == "dense":
        for fam in lens:
            assert lens[fam][-1] >= (129 if c.S == 8300 else 65), (c.id, fam, lens[fam])
    edges, info = long_edges(m4, c.S, c.Hq, c.Hkv, c.causal, lists)
    if white:
        from golden_util import make_inputs, round_to
        q, k, v, do = (round_to(x, c.dt) for x in make_inputs(1, c.S, c.Hq, c.Hkv, c.D, seed=c.S + c.D))
        nd = SimpleNamespace(q=q, k=k, v=v, do=do)
    else:
        nd = NI.make(c.S, c.S, c.Hq, c.Hkv, c.D, c.dt, C=8, seed=c.S % 97, B=1, edges=edges)
    built = SimpleNamespace(mask=mask, m4=m4, lists=lists, lens=lens, edges=edges, info=info, nd=nd)
    _LONG_BUILT[key] = built
    return built


def long_needle_conditions(c, built, n_rows=12):
    """needle_inputs.assert_needle_conditions per query head (the mask differs from head to head), `visible` from
    block_mask_ref.visible: on the named rows and a seeded draw."""
    G = c.G
    m4 = torch.from_numpy(built.m4)
    rows = sorted(set(list(built.info.ids)[:n_rows]) | set(int(x) for x in np.random.RandomState(5).randint(0, c.S, size=n_rows)))
    nd = built.nd
    res = []
    for h in range(c.Hq):
        one = SimpleNamespace(q=nd.q[:, :, h:h + 1], k=nd.k[:, :, h // G:h // G + 1], kdir=nd.kdir[:, h // G:h // G + 1],
                              qdir=nd.qdir[:, h:h + 1])
        vis = lambda r: R.visible(m4, 0, r, r + 1, c.S, c.causal)[h, 0].numpy()
        res.append(NI.assert_needle_conditions(one, rows, c.D ** -0.5, vis, what=f"{c.id} head {h}"))
    return res


def lost_block_mutations(c, built):
    """Three single-bit mutations of a S = 4400 case's mask, each clearing the bit of an edge-needled block ->
    {name: (head, row block, key block, list position of the block's first lost tile)}: `fwd` -- the lost tiles sit as far back as
    the case allows in the dQ list of a sampled row block's pair (and in its forward list); `transposed` -- likewise in the
    transposed list of a sampled key block; `last` -- the one-tile last key block.  The position is >= 64 wherever the case has
    such a list: every `dense` case and circ33; circ32 for `fwd` only (its dQ lists hold 65 / 66 entries, its forward and
    transposed ones 63 / 64); circ31 has no list past 64 entries and takes its last positions."""
    nb = built.m4.shape[-1]
    pick = {}
    for fam, blk, h, pos, row, key in built.info.records:
        r, kb = row // BLOCK, key // BLOCK
        if kb == nb - 1:
            if one_tile_last_block(c.S):
                pick.setdefault("last", (h, r, kb, pos))
            continue
        if fam == "fwd":
            where = [e // 4 for e in built.lists["dq"][0, h, r // 2]].index(2 * kb)
            if where > pick.get("fwd", (0, 0, 0, -1))[3]:
                pick["fwd"] = (h, r, kb, where)
        elif r != nb - 1:
            where = built.lists["dkdv"][0, h, kb].index(2 * r)
            if where > pick.get("transposed", (0, 0, 0, -1))[3]:
                pick["transposed"] = (h, r, kb, where)
    assert set(pick) == {"fwd", "transposed", "last"}, (c.id, sorted(pick))
    floor = {"fwd": 60 if c.kind == "circ31" else 64, "transposed": 60 if c.kind in ("circ31", "circ32") else 64}
    for name, least in floor.items():
        assert pick[name][3] >= least, (c.id, name, pick[name])
    return pick


# ------------------------------------------------------------------------------------------------------------------------------
# HEADS
# ------------------------------------------------------------------------------------------------------------------------------
HEADS_S, HEADS_B, HEADS_D, HEADS_DT = 384, 2, 64, "bfloat16"
HEAD_PATTERNS = ("first", "middle", "last", "all_but_last", "all_but_first", "all")


def empty_heads(pattern, G):
    """The heads of a group (0 ... G - 1) whose transposed list is empty under `pattern`."""
    return {"first": {0}, "middle": {G // 2}, "last": {G - 1}, "all_but_last": set(range(G - 1)), "all_but_first": set(range(1, G)),
            "all": set(range(G))}[pattern]


def heads_mask(Hq, Hkv, causal, seed=0):
    """(mask (B, Hq, 3, 3), {(b, kv head, key block): pattern}): slot (b, c) of KV head hk carries pattern (3 b + c + 2 hk) mod 6.
    A head whose list is empty has its column all false; every other head's column is seeded at 0.5 with its diagonal block set,
    which the causal cut leaves alive -- so all six patterns survive under causal (asserted: at least four)."""
    B, nb, G = HEADS_B, R.n_blocks(HEADS_S), Hq // Hkv
    rs = np.random.RandomState(7000 + Hq + seed)
    m = rs.rand(B, Hq, nb, nb) < 0.5
    m[:, :, np.arange(nb), np.arange(nb)] = True
    slots = {}
    for b in range(B):
        for c in range(nb):
            for hk in range(Hkv):
                pat = HEAD_PATTERNS[(nb * b + c + 2 * hk) % 6]
                slots[b, hk, c] = pat
                for g in empty_heads(pat, G):
                    m[b, hk * G + g, :, c] = False
    lists = R.enumerate_lists(m, HEADS_S, causal)
    alive = set()
    for (b, hk, c), pat in slots.items():
        got = {g for g in range(G) if not lists["dkdv"][b, hk * G + g, c]}
        assert got == empty_heads(pat, G), (Hq, Hkv, causal, b, hk, c, pat, got)
        alive.add(pat)
    assert len(alive) >= 4
    return m, slots


def heads_cases():
    return [SimpleNamespace(S=HEADS_S, B=HEADS_B, Hq=Hq, Hkv=Hkv, D=HEADS_D, dt=HEADS_DT, causal=causal, G=Hq // Hkv,
                            id=f"H{Hq}/{Hkv}-{'causal' if causal else 'full'}")
            for Hq, Hkv in ((4, 1), (6, 2)) for causal in (True, False)]


HEADS = heads_cases()


def divisors_with_zero(G, among=(0, 1, 2)):
    """dkdv_heads in {0, 1, 2, G}, only divisors of G (0: the library decides)."""
    return sorted(set(x for x in among + (G,) if x == 0 or G % x == 0))


# ------------------------------------------------------------------------------------------------------------------------------
# the fuzz sweep
# ------------------------------------------------------------------------------------------------------------------------------
FUZZ_BASE = 31009                        # its first 24 seeds: 14 with a one-tile last block, 4 non-contiguous masks, 14 with G >= 3 and dkdv_heads < G
FUZZ_DEFAULT = 24
FUZZ_HEADS = [(1, 1), (3, 1), (4, 2), (6, 2), (8, 1)]
FUZZ_FORMS = ("2d", "3d", "4d", "window")


def fuzz_case(seed):
    """One case of test_fuzz_block_mask: S in [1, 700], B, the heads, D, dtype, causal, the mask's density and form (`window`: a
    strided window of a larger mask -- non-contiguous), dkdv_heads (a divisor of G).  `mask`: the numpy mask in the drawn form;
    `m4`: its (B, Hq, nb, nb) expansion.  `rs` goes on to draw the layouts."""
    rs = np.random.RandomState(FUZZ_BASE + seed)
    S = int(rs.randint(1, 701))
    B = int(rs.choice([1, 2, 3]))
    Hq, Hkv = FUZZ_HEADS[int(rs.randint(len(FUZZ_HEADS)))]
    D = int(rs.choice([32, 64, 128]))
    dt = str(rs.choice(DTYPES))
    causal = bool(rs.rand() < 0.5)
    density = float(rs.choice([0.1, 0.5, 0.9]))
    form = str(rs.choice(FUZZ_FORMS))
    G = Hq // Hkv
    heads = int(rs.choice([g for g in range(1, G + 1) if G % g == 0]))
    nb = R.n_blocks(S)
    shape = {"2d": (nb, nb), "3d": (Hq, nb, nb)}.get(form, (B, Hq, nb, nb))
    mask = rs.rand(*shape) < density
    what = f"bsp seed {seed} B{B} S{S} Hq{Hq} Hkv{Hkv} D{D} {dt} causal={causal} density={density} form={form} dkdv_heads={heads}"
    return SimpleNamespace(rs=rs, seed=seed, S=S, B=B, Hq=Hq, Hkv=Hkv, D=D, dt=dt, causal=causal, density=density, form=form, G=G,
                           heads=heads, mask=mask, m4=np.array(m4_of(mask, B, Hq)), what=what)


def fuzz_coverage(n=FUZZ_DEFAULT):
    """What the first n seeds reach, from the generator alone."""
    cs = [fuzz_case(s) for s in range(n)]
    return dict(one_tile_last_block=sum(one_tile_last_block(c.S) for c in cs),
                non_contiguous_mask=sum(c.form == "window" for c in cs),
                head_walk_split=sum(c.G >= 3 and c.heads < c.G for c in cs))
