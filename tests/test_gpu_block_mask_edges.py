"""Block-sparse attention (block_mask=) at the places tests/test_gpu_block_mask.py does not reach: sequence ends whose last block
has one 64-tile (the builder's `second` branch, the kernels' clamps on a list that ends in a one-tile block), lists past 64 and 128
entries (dQ's 64-entry refill, the forward's ballot per 64 entries), the dK/dV head walk with stated empty heads, `only=` and
`accum_*` launches, and every tensor of a call in a memory layout of its own.  The cases are tests/block_mask_inputs.py's; the
reference is tests/block_mask_ref.py (fp64, on the device, the mask from its definition alone); the tolerances are the project's:
golden_util.TOL / grad_tol, the lse at 2e-3 + 1e-4 |lse|, needle_inputs.verdicts on the needle cases.

Each comparison prints its worst error as a fraction of its bound ("[bsp-edges]") before it asserts; profiles/block_mask_edges.txt
records those lines."""
import os

import numpy as np
import pytest
import torch

import block_mask_inputs as BI
import block_mask_ref as R
import layout_util as LU
import needle_inputs as NI
from golden_util import TOL, assert_close, grad_tol, make_inputs

pytestmark = pytest.mark.gpu

LSE_TOL = (2e-3, 1e-4)
POISON = -7
NAMES = ("out", "lse", "dq", "dk", "dv")
_N_FUZZ = int(os.environ.get("USP_FUZZ_BSP", str(BI.FUZZ_DEFAULT)))          # larger sweeps: USP_FUZZ_BSP=400


@pytest.fixture(scope="module")
def dev():
    from yunchang_amd import _C
    _C.load()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _dev16(x, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(getattr(torch, dt)).to(dev)


_WHITE = {}


def white(dev, B, S, Hq, Hkv, D, dt):
    key = (B, S, Hq, Hkv, D, dt)
    if key not in _WHITE:
        _WHITE[key] = [_dev16(x, dt, dev) for x in make_inputs(B, S, Hq, Hkv, D, seed=S + D)]
    return _WHITE[key]          # q, k, v, dout


def poisoned_lists(dev, B, Hq, S):
    from yunchang_amd import _C
    nb = R.n_blocks(S)
    lay = _C.block_list_layout(B, Hq, nb)
    assert _C.block_list_bytes(B, Hq, nb) == 4 * lay["ints"]
    return torch.full((lay["ints"],), POISON, dtype=torch.int32, device=dev), lay


def launch(q, k, v, do, mask, causal, lists=None, interleave=False, dkdv_heads=0):
    """Forward, delta and backward through the C ABI -> (out, lse, dq, dk, dv), the gradients in fp32; every output NaN-filled."""
    from yunchang_amd import _C
    B, S, Hq, D = q.shape
    out = torch.full_like(q, float("nan"))
    lse = torch.full((B, Hq, S), float("nan"), dtype=torch.float32, device=q.device)
    _C.flash_fwd(q, k, v, D ** -0.5, causal, lse, out=out, bsp=mask, bsp_lists=lists, interleave=interleave)
    delta = torch.empty_like(lse)
    _C.bwd_delta(do, out, delta)
    dq, dk, dv = (torch.full(t.shape, float("nan"), dtype=torch.float32, device=q.device) for t in (q, k, v))
    _C.flash_bwd(do, q, k, v, lse, delta, dq, dk, dv, D ** -0.5, causal, bsp=mask, bsp_lists=lists, interleave=interleave,
                 dkdv_heads=dkdv_heads)
    return out, lse, dq, dk, dv


def check_lists(lists, lay, want, Hq, what, families=("fwd", "dq", "dkdv")):
    """The lists read back against the enumeration: counts and entries, and the rest of every list's slot still poison."""
    got = lists.cpu().numpy()
    for fam in families:
        off, per, stride = lay[fam]
        for (b, h, i), ent in want[fam].items():
            base = off + ((b * Hq + h) * per + i) * stride
            assert got[base] == len(ent), (what, fam, b, h, i, got[base], len(ent))
            assert list(got[base + 1:base + 1 + len(ent)]) == ent, (what, fam, b, h, i)
            assert (got[base + 1 + len(ent):base + stride] == POISON).all(), (what, fam, b, h, i, "written past the count")


def check(got, ref, dt, G, what):
    """Every element at the stated tolerances; prints the worst err / bound per tensor first."""
    tols = [TOL[dt]["out"], LSE_TOL] + [grad_tol(dt, G)] * 3
    ratios = [NI.bound_ratio(g, r, *t)[1] for g, r, t in zip(got, ref, tols)]
    print(f"[bsp-edges] {what}: " + " ".join(f"{n}={x:.3f}" for n, x in zip(NAMES, ratios)))
    for g, r, t, n in zip(got, ref, tols, NAMES):
        assert_close(g, r, *t, f"{what} {n}")
    return ratios


def check_dead_rows(got, ref, what):
    """Rows that see nothing: exactly out = 0, lse = -inf, dq = 0."""
    dead = torch.isinf(ref[1])
    assert bool((got[1][dead] == float("-inf")).all()), what
    assert bool((got[0].transpose(1, 2)[dead] == 0).all()) and bool((got[2].transpose(1, 2)[dead] == 0).all()), what
    return int(dead.sum())


# ---- 1. sequence ends -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("S", BI.RAGGED_S)
def test_ragged_ends(dev, S, causal):
    """Every RAGGED case of this S: forward and backward against the reference, rows that see nothing exactly 0 / -inf / 0, the
    built lists read back from a poisoned workspace.  Where S mod 128 lies in (0, 64] the all-set case's lists must end in the
    one-tile block: the last entry is tile 2 (nb - 1) and the count is odd."""
    cases = [c for c in BI.RAGGED if c.S == S and c.causal == causal]
    assert len(cases) == 16
    nb = R.n_blocks(S)
    n_dead = 0
    for c in cases:
        q, k, v, do = white(dev, c.B, S, c.Hq, c.Hkv, c.D, c.dt)
        m = BI.ragged_mask(c.kind, c.B, c.Hq, S)
        mask = torch.from_numpy(m).to(dev)
        ref = R.ref_all(do, q, k, v, c.D ** -0.5, mask, causal)
        lists, lay = poisoned_lists(dev, c.B, c.Hq, S)
        got = launch(q, k, v, do, mask, causal, lists=lists)
        check(got, ref, c.dt, c.Hq // c.Hkv, c.id)
        n_dead += check_dead_rows(got, ref, c.id)
        want = R.enumerate_lists(m, S, causal)
        check_lists(lists, lay, want, c.Hq, c.id)
        if BI.one_tile_last_block(S) and c.kind == "all":
            flat = lists.cpu().numpy()
            for fam, tile in (("fwd", 2 * (nb - 1)), ("dq", 4 * 2 * (nb - 1) + (1 if nb % 2 else (2 if causal else 3))), ("dkdv", 2 * (nb - 1))):
                off, per, stride = lay[fam]
                base = off + (per - 1) * stride                      # (b 0, head 0, the last row block / pair / key block)
                assert flat[base] % 2 == 1 and flat[base + flat[base]] == tile, (c.id, fam, flat[base:base + stride])
    print(f"[bsp-edges] S{S} causal={causal}: {len(cases)} cases, {n_dead} (b, h, row) entries that see nothing")


# ---- 2. lists past 64 and 128 entries --------------------------------------------------------------------------------------------
_LONG = {}


def long_on_device(dev, c):
    """(q, k, v, dout, the mask as handed over, the fp64 reference as a dict) of a LONG case; computed once."""
    if c.id not in _LONG:
        b = BI.long_build(c)
        t = [_dev16(x, c.dt, dev) for x in (b.nd.q, b.nd.k, b.nd.v, b.nd.do)]
        mask = torch.from_numpy(np.array(b.mask)).to(dev)
        ref = dict(zip(NAMES, R.ref_all(t[3], t[0], t[1], t[2], c.D ** -0.5, mask, c.causal)))
        _LONG[c.id] = (t, mask, ref, b)
    return _LONG[c.id]


def judge(got, ref, c, what):
    """needle_inputs.verdicts on (out, lse, dq, dk, dv); prints the ratios."""
    v = NI.verdicts(dict(zip(NAMES, got)), ref, c.dt, c.S, c.S, c.G)
    print(f"[bsp-edges] {what}: " + " ".join(f"{n}={v[n][1]:.3f}" for n in NAMES))
    return v


@pytest.mark.parametrize("c", BI.LONG, ids=lambda c: c.id)
def test_long_lists(dev, c):
    """A LONG case through _C.flash_fwd / bwd_delta / flash_bwd, once persistent and once with interleave=True (bit-identical),
    every element judged by needle_inputs.verdicts, the lists read back."""
    (q, k, v, do), mask, ref, b = long_on_device(dev, c)
    print(f"[bsp-edges] {c.id}: list lengths " + " ".join(f"{f}={l[0]}..{l[-1]}" for f, l in b.lens.items()) + f", {len(b.edges)} edge needles")
    if c.kind == "dense":
        assert all(l[-1] >= (129 if c.S == 8300 else 65) for l in b.lens.values()), b.lens
    res = []
    for interleave in (False, True):
        lists, lay = poisoned_lists(dev, 1, c.Hq, c.S)
        res.append(launch(q, k, v, do, mask, c.causal, lists=lists, interleave=interleave))
        check_lists(lists, lay, b.lists, c.Hq, c.id)
    for n, x, y in zip(NAMES, *res):
        assert torch.equal(x, y), f"{c.id}: {n} differs between the persistent and the interleaved launch"
    verdict = judge(res[0], ref, c, c.id)
    assert all(ok for ok, _ in verdict.values()), (c.id, verdict)
    check_dead_rows(res[0], [ref[n] for n in NAMES], c.id)


@pytest.mark.parametrize("c", [c for c in BI.LONG if c.S == 4400], ids=lambda c: c.id)
def test_long_lists_see_one_lost_block(dev, c):
    """Test power on the device: the kernels get the mask with ONE bit of an edge-needled block cleared, the reference keeps the
    true mask -- an ordinary launch under another valid mask.  out and lse must fail for each of the three mutations; dq for the
    one at the back of a dQ list, dk and dv for the one at the back of a transposed list."""
    (q, k, v, do), _, ref, b = long_on_device(dev, c)
    for name, (h, r, kb, pos) in sorted(BI.lost_block_mutations(c, b).items()):
        m = b.m4.copy()
        assert m[0, h, r, kb]
        m[0, h, r, kb] = False
        got = launch(q, k, v, do, torch.from_numpy(m).to(dev), c.causal)
        verdict = judge(got, ref, c, f"{c.id} lost block ({name}: head {h}, row block {r}, key block {kb}, list position {pos})")
        must = ("out", "lse") + {"fwd": ("dq",), "transposed": ("dk", "dv"), "last": ()}[name]
        for n in must:
            assert not verdict[n][0], f"{c.id}: {n} does not see the block lost by mutation `{name}`: {verdict}"


# ---- 3. the dK/dV head walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", BI.HEADS, ids=lambda c: c.id)
def test_head_walks(dev, c):
    """HEADS cases with dkdv_heads in {0, 1, 2, G} (divisors of G): against the reference; dK / dV of a key block whose lists are
    empty for every head of the group exactly 0; only="dq" / only="dkdv" bit-identical to the combined call, the other outputs'
    NaN fill and the other family's region of the poisoned workspace untouched; accum_dq / accum_dk / accum_dv on preset fp32
    buffers: preset + gradient within grad_tol, rows and key blocks with empty lists keep the preset bit for bit."""
    from yunchang_amd import _C
    B, S, Hq, Hkv, D, G = c.B, c.S, c.Hq, c.Hkv, c.D, c.G
    q, k, v, do = white(dev, B, S, Hq, Hkv, D, c.dt)
    m, slots = BI.heads_mask(Hq, Hkv, c.causal)
    mask = torch.from_numpy(m).to(dev)
    want_lists = R.enumerate_lists(m, S, c.causal)
    ref = R.ref_all(do, q, k, v, D ** -0.5, mask, c.causal)
    scale = D ** -0.5
    blind = [(b, hk, kb) for (b, hk, kb), pat in slots.items() if pat == "all"]
    assert blind
    dead = torch.isinf(ref[1]).transpose(1, 2)                                        # (B, S, Hq)
    for heads in BI.divisors_with_zero(G):
        what = f"{c.id} dkdv_heads={heads}"
        lists, lay = poisoned_lists(dev, B, Hq, S)
        got = launch(q, k, v, do, mask, c.causal, lists=lists, dkdv_heads=heads)
        check(got, ref, c.dt, G, what)
        check_lists(lists, lay, want_lists, Hq, what)
        check_dead_rows(got, ref, what)
        out, lse, dq, dk, dv = got
        for b, hk, kb in blind:
            for t in (dk, dv):
                assert bool((t[b, 128 * kb:128 * (kb + 1), hk] == 0).all()), (what, b, hk, kb)
        delta = torch.empty_like(lse)
        _C.bwd_delta(do, out, delta)
        # only="dq" / only="dkdv": what they write, what they leave
        for only, live, fams in (("dq", (0,), ("dq",)), ("dkdv", (1, 2), ("dkdv",))):
            lists2, _ = poisoned_lists(dev, B, Hq, S)
            g = [torch.full(t.shape, float("nan"), dtype=torch.float32, device=dev) for t in (q, k, v)]
            _C.flash_bwd(do, q, k, v, lse, delta, *g, scale, c.causal, bsp=mask, bsp_lists=lists2, dkdv_heads=heads, only=only)
            for i, n in enumerate(("dq", "dk", "dv")):
                if i in live:
                    assert torch.equal(g[i], got[2 + i]), f"{what}: {n} of only={only} differs from the combined call"
                else:
                    assert bool(torch.isnan(g[i]).all()), f"{what}: only={only} wrote {n}"
            check_lists(lists2, lay, want_lists, Hq, what, families=fams)
            flat = lists2.cpu().numpy()
            for fam in ("fwd", "dq", "dkdv"):
                if fam not in fams:
                    off, per, stride = lay[fam]
                    assert (flat[off:off + B * Hq * per * stride] == POISON).all(), f"{what}: only={only} wrote the {fam} lists"
        # accum_*: preset + gradient
        gen = torch.Generator(device="cpu").manual_seed(17 + heads)
        preset = [torch.randn(t.shape, generator=gen, dtype=torch.float32).to(dev) for t in (q, k, v)]
        g = [p.clone() for p in preset]
        _C.flash_bwd(do, q, k, v, lse, delta, *g, scale, c.causal, accum_dq=True, accum_dk=True, accum_dv=True, bsp=mask,
                     dkdv_heads=heads)
        for t, p, r_, n in zip(g, preset, ref[2:], ("dq", "dk", "dv")):
            assert_close(t, p.double() + r_, *grad_tol(c.dt, G), f"{what} accum {n}")
        assert bool(dead.any())
        assert torch.equal(g[0][dead].view(torch.int32), preset[0][dead].view(torch.int32)), f"{what}: accum_dq changed a row with an empty list"
        for b, hk, kb in blind:
            for t, p in zip(g[1:], preset[1:]):
                rows = slice(128 * kb, 128 * (kb + 1))
                assert torch.equal(t[b, rows, hk].view(torch.int32), p[b, rows, hk].view(torch.int32)), (what, "accum", b, hk, kb)


# ---- 4. two launches, the second with every tensor in a layout of its own ---------------------------------------------------------
GUARD = 64                                                          # int32 words on either side of the lists workspace


def two_launches(dev, what, tensors, mask_first, m4, causal, dt, heads, rs, judge_with=None):
    """Launch 1: contiguous tensors, `mask_first`.  Launch 2: interleave=True, q, k, v, dout, out, lse, the lse input, delta and
    dq16 / dk16 / dv16 each an independently drawn strided view inside one sentinel arena, the mask a strided window of a larger
    one, the lists workspace exactly block_list_bytes between guard words.  Required: both launches bit-identical, nothing written
    outside the views, the inputs unchanged, the guards intact, the lists those of the enumeration; launch 1 within tolerance."""
    from yunchang_amd import _C
    q, k, v, do = tensors
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    G, nb, scale, dtype = Hq // Hkv, R.n_blocks(S), D ** -0.5, q.dtype
    want_lists = R.enumerate_lists(m4, S, causal)
    # ---- launch 1
    lists1, lay = poisoned_lists(dev, B, Hq, S)
    out = torch.full_like(q, float("nan"))
    lse = torch.full((B, Hq, S), float("nan"), dtype=torch.float32, device=dev)
    _C.flash_fwd(q, k, v, scale, causal, lse, out=out, bsp=mask_first, bsp_lists=lists1)
    delta = torch.full_like(lse, float("nan"))
    _C.bwd_delta(do, out, delta)
    g1 = [torch.full_like(t, float("nan")) for t in (q, k, v)]
    _C.flash_bwd(do, q, k, v, lse, delta, None, None, None, scale, causal, dq16=g1[0], dk16=g1[1], dv16=g1[2], bsp=mask_first,
                 bsp_lists=lists1, dkdv_heads=heads)
    check_lists(lists1, lay, want_lists, Hq, what)
    # ---- launch 2
    lay_of = lambda name: LU.draw_layout(rs, LU.ROLE[name], B)
    arena = LU.Arena(dev)
    sq, sk, sv, sdo = (LU.place(t, lay_of(n), arena, n) for t, n in ((q, "q"), (k, "k"), (v, "v"), (do, "dout")))
    out2 = LU.blank((B, S, Hq, D), dtype, lay_of("out"), arena, "out")
    lse2 = LU.blank((B, Hq, S), torch.float32, lay_of("lse"), arena, "lse")
    big = torch.from_numpy(rs.rand(B, Hq + 1, 2 * nb, 2 * nb + 1) < 0.5).to(dev)
    big[:, 1:, nb:, 1:nb + 1] = torch.from_numpy(np.array(m4)).to(dev)
    big_before = big.clone()
    mask2 = big[:, 1:, nb:, 1:nb + 1]
    assert not mask2.is_contiguous() or nb == 1 and B == 1 and Hq == 1
    buf = torch.full((lay["ints"] + 2 * GUARD,), POISON, dtype=torch.int32, device=dev)
    lists2 = buf[GUARD:GUARD + lay["ints"]]
    assert lists2.numel() * 4 == _C.block_list_bytes(B, Hq, nb)
    _C.flash_fwd(sq, sk, sv, scale, causal, lse2, out=out2, bsp=mask2, bsp_lists=lists2, interleave=True)
    LU.assert_same_bits(out, out2, what + ": out")
    LU.assert_same_bits(lse, lse2, what + ": lse")
    slse = LU.place(lse, lay_of("lse"), arena, "lse_in")
    sdelta = LU.blank((B, Hq, S), torch.float32, lay_of("delta"), arena, "delta")
    so = LU.place(out, lay_of("o"), arena, "o")                      # (delta's `out` is a 16-bit INPUT: 16-byte aligned, unlike out2)
    _C.bwd_delta(sdo, so, sdelta)
    LU.assert_same_bits(delta, sdelta, what + ": delta")
    g2 = [LU.blank(tuple(t.shape), dtype, lay_of(n), arena, n) for t, n in ((q, "dq16"), (k, "dk16"), (v, "dv16"))]
    _C.flash_bwd(sdo, sq, sk, sv, slse, sdelta, None, None, None, scale, causal, dq16=g2[0], dk16=g2[1], dv16=g2[2], bsp=mask2,
                 bsp_lists=lists2, interleave=True, dkdv_heads=heads)
    for a_, b_, n_ in zip(g1, g2, ("dq", "dk", "dv")):
        LU.assert_same_bits(a_, b_, f"{what}: {n_}")
    bad = arena.violations()
    assert not bad, f"{what}: written outside the views: {bad}"
    assert arena.unchanged(), what + ": an input view was modified"
    assert torch.equal(big, big_before), what + ": the mask was modified"
    assert bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + lay["ints"]:] == POISON).all()), what + ": the lists' guard words were written"
    check_lists(lists2, lay, want_lists, Hq, what)
    # ---- launch 1 against the reference
    got = (out, lse) + tuple(g1)
    if judge_with is not None:
        c, ref = judge_with
        verdict = judge(got, ref, c, what)
        assert all(ok for ok, _ in verdict.values()), (what, verdict)
        ref = [ref[n] for n in NAMES]
    else:
        ref = R.ref_all(do, q, k, v, scale, torch.from_numpy(np.array(m4)).to(dev), causal)
        check(got, ref, dt, G, what)
    check_dead_rows(got, ref, what)


@pytest.mark.parametrize("seed", range(_N_FUZZ))
def test_fuzz_block_mask(dev, seed):
    """The seeded sweep of tests/block_mask_inputs.py:fuzz_case, white noise, through two_launches."""
    c = BI.fuzz_case(seed)
    tensors = [_dev16(x, c.dt, dev) for x in make_inputs(c.B, c.S, c.Hq, c.Hkv, c.D, seed=seed)]
    nb = R.n_blocks(c.S)
    if c.form == "window":               # a strided window of a larger mask
        big = torch.from_numpy(c.rs.rand(c.B, c.Hq + 2, nb + 3, 2 * nb + 5) < 0.5).to(dev)
        big[:, 2:, 3:, 2:nb + 2] = torch.from_numpy(c.mask).to(dev)
        first = big[:, 2:, 3:, 2:nb + 2]
        assert first.stride(-1) == 1 and first.stride(-2) == 2 * nb + 5
    else:
        first = torch.from_numpy(c.mask).to(dev)
    two_launches(dev, c.what, tensors, first, c.m4, c.causal, c.dt, c.heads, c.rs)


@pytest.mark.parametrize("which", ["long"] + [c.id for c in BI.HEADS])
def test_second_launch_of_the_long_and_head_cases(dev, which):
    """One LONG S = 4400 case (`dense`, causal, D = 128, G = 2) and the HEADS cases through the same two launches."""
    rs = np.random.RandomState(8000 + len(which))
    if which == "long":
        c = BI.LONG[0]
        assert c.S == 4400 and c.kind == "dense"
        tensors, mask, ref, b = long_on_device(dev, c)
        two_launches(dev, c.id + " (two launches)", tensors, mask, b.m4, c.causal, c.dt, 1, rs, judge_with=(c, ref))
        return
    c = [x for x in BI.HEADS if x.id == which][0]
    m, _ = BI.heads_mask(c.Hq, c.Hkv, c.causal)
    tensors = white(dev, c.B, c.S, c.Hq, c.Hkv, c.D, c.dt)
    two_launches(dev, c.id + " (two launches)", tensors, torch.from_numpy(m).to(dev), m, c.causal, c.dt, 1, rs)
