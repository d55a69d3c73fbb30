"""The dropout mask read-out (tests/mask_readout.py) without a GPU: every problem of the builder, solved by tests/dropout_ref.py
in fp64, decodes to keep_mask & visible exactly -- also with a window and a shift, far offsets and several passes -- and mutants of
the mask (the references' `keep=` override) decode to exactly the set of differing positions: the decoder localises.  The
counterpart of tests/test_dropout_cpu.py::test_mutant_references_are_far_away, which shows what the tolerances see."""
import numpy as np
import pytest
import torch

import dropout_ref
import mask_readout as MR
from shift_ref import visible

SEED = (1 << 40) + 1234
FAR = ((1 << 31) - 208, (1 << 20) + 8, 5)


def _solve(kind, s, p, passes, at, causal, window, shift, keep=None):
    """The tensor that carries the bits, per pass, by the fp64 reference; asserts the outputs that must be exactly zero."""
    res = []
    lse, _ = MR.stats(s)
    kw = dict(causal=causal, window=window, shift=shift, keep=keep)
    for ps in passes:
        if kind == "fwd":
            res.append(dropout_ref.ref_fwd(ps.q, ps.k, ps.v, MR.SCALE, p, SEED, at, **kw)[0])
            continue
        zero_out = torch.zeros_like(ps.q)                                       # delta = rowsum(dout * out) = 0
        dq, dk, dv = dropout_ref.ref_bwd_from(ps.dout, ps.q, ps.k, ps.v, zero_out, lse, MR.SCALE, p, SEED, at, **kw)
        zero = {"dq": (dk,), "dk": (dq,), "dv": (dq, dk)}[kind]
        assert all(bool((z == 0).all()) for z in zero), kind
        res.append({"dq": dq, "dk": dk, "dv": dv}[kind])
    return res


def _readout(kind, s, p, at=(0, 0, 0), causal=False, window=None, shift=0, keep=None, **kw):
    passes = MR.build(kind, s, p, **kw)
    vis = visible(s.Sq, s.Sk, causal, window, shift).numpy()
    return MR.decode(kind, s, p, passes, _solve(kind, s, p, passes, at, causal, window, shift, keep), vis) + (len(passes),)


# the block shape of tests/test_gpu_dropout_readout.py at D 32 (Sq % 4 = 3, Sk % 4 = 2, 8 key planes, 2 x 7 row planes), and a
# shrunk D 64 one (fp64 on the CPU): 4 key planes, 2 x 2 row planes, more than one 64-key tile
SHAPES = [MR.Shape(2, 203, 254, 4, 2, 32, "bfloat16"), MR.Shape(2, 203, 254, 4, 2, 32, "float16"), MR.Shape(1, 75, 250, 4, 2, 64, "float16")]


@pytest.mark.parametrize("kind", MR.KINDS)
@pytest.mark.parametrize("s", SHAPES, ids=lambda s: f"D{s.D}-{s.dt}")
def test_reference_decodes_to_the_mask(s, kind):
    for i, (p, t) in enumerate(MR.PROBS.items()):
        assert dropout_ref.threshold(p) == t
        at, causal = ((0, 0, 0), FAR)[i % 2], bool(i % 3 == 0)
        bits, dev, n = _readout(kind, s, p, at, causal)
        want = MR.expected(s, p, SEED, at, causal)
        assert MR.compare(bits, want, at, f"{kind} p {p} at {at}") == want.size
        assert dev < 1e-9, dev                                             # fp64: zero deviation from an integer
        pow2 = t & (t - 1) == 0
        assert n == (1 if kind != "dq" or pow2 else -(-len(MR.all_planes(kind, s)) // {"bfloat16": 4, "float16": 6}[s.dt])), n


@pytest.mark.parametrize("kind", MR.KINDS)
@pytest.mark.parametrize("causal,window,shift", [(True, (70, 0), 0), (False, (100, 40), 0), (True, None, -37), (True, None, 64),
                                                 (False, (17, 3), -5)])
def test_window_and_shift(kind, causal, window, shift):
    s, p = SHAPES[0], 0.1
    bits, dev, _ = _readout(kind, s, p, FAR, causal, window, shift)
    want = MR.expected(s, p, SEED, FAR, causal, window, shift)
    assert want.any() and not want.all()
    MR.compare(bits, want, FAR, f"{kind} causal {causal} window {window} shift {shift}")
    assert dev < 1e-9


def test_merged_and_out16_passes_hold_few_planes():
    s = SHAPES[0]
    assert [len(ps.planes) for ps in MR.build("fwd", s, 0.1, merged=True)] == [8]
    assert [len(ps.planes) for ps in MR.build("fwd", s, 0.1, out16=True)] == [4, 4]
    assert [len(ps.planes) for ps in MR.build("dq", s, 0.1)] == [4, 4] and [len(ps.planes) for ps in MR.build("dq", s, 0.75)] == [8]
    assert [len(ps.planes) for ps in MR.build("dq", SHAPES[1], 0.9)] == [6, 2]
    wide = MR.Shape(1, 32 * 12, 8, 4, 2, 32, "float16")                    # 2 x 12 row planes: two passes, exponents from below 0
    ps = MR.build("dk", wide, 0.5)
    assert [len(x.planes) for x in ps] == [16, 8] and ps[0].lo == -1 and float(ps[0].q.float().max()) == 2.0 ** 14
    bits, dev, n = _readout("dk", wide, 0.5)
    MR.compare(bits, MR.expected(wide, 0.5, SEED), what="two passes of row planes")
    # a 16-bit `out`: the rounded forward result still decodes at 4 planes
    for s16 in SHAPES[:2]:
        passes = MR.build("fwd", s16, 0.1, out16=True)
        vis = visible(s16.Sq, s16.Sk, True).numpy()
        outs = [r.to(getattr(torch, s16.dt)) for r in _solve("fwd", s16, 0.1, passes, FAR, True, None, 0)]
        bits, dev = MR.decode("fwd", s16, 0.1, passes, outs, vis)
        MR.compare(bits, MR.expected(s16, 0.1, SEED, FAR, True), FAR, "16-bit out")
        assert dev <= 1.0 / 16                                             # x < 16, rounded at 2^-8 relative (bf16)
        bits, _ = MR.decode("fwd", s16, 0.1, passes, outs, vis, rows=slice(50, 150))        # a row range
        want = MR.expected(s16, 0.1, SEED, FAR, True)
        assert np.array_equal(bits[:, :, 50:150, :s16.Sk], want[:, :, 50:150]) and not bits[:, :, :50].any() and not bits[:, :, 150:].any()


def _mutants(s, p, at, true):
    """name -> wrong keep mask (B, Hq, Sq, Sk) bool."""
    B, Hq, Sq, Sk = true.shape
    t = dropout_ref.threshold(p)
    out = {}
    m = true.copy()
    m[1, 2, 177, 201] ^= True                                              # (positions a causal mask still shows)
    out["one flipped bit"] = m
    m = true.copy()
    m[0, 1, 100:104, 64:68] = true[0, 1, 100:104, 64:68].T
    out["one transposed patch"] = m
    m = true.copy()
    m[1, 2, 160:192, 128:192] = true[1, 3, 160:192, 128:192]
    out["a 32 x 64 block of the head beside it"] = m
    by = dropout_ref.keep_bytes(SEED, B, Hq, Sq + 4, Sk + 64, *at)
    m = true.copy()
    m[0, 0, 64:96] = by[0, 0, 68:100, :Sk] < t
    out["rows displaced by 4"] = m
    m = true.copy()
    k0 = Sk // 64 * 64                                                     # the last, ragged tile
    m[:, :, Sq - 32:, k0:] = by[:, :, Sq - 32:Sq, k0 + 64:Sk + 64] < t
    out["keys displaced by 64 in the last ragged tile"] = m
    return out


@pytest.mark.parametrize("kind", MR.KINDS)
@pytest.mark.parametrize("causal", [False, True])
def test_mutants_decode_to_exactly_the_differing_positions(kind, causal):
    s, p, at = SHAPES[0], 0.5, ((1 << 20) + 4, 8, 5)
    true = dropout_ref.keep_mask(p, SEED, s.B, s.Hq, s.Sq, s.Sk, *at)
    vis = visible(s.Sq, s.Sk, causal).numpy()
    want = MR.expected(s, p, SEED, at, causal)
    for name, m in _mutants(s, p, at, true).items():
        keep = (torch.from_numpy(m).double(), dropout_ref.rescale(p))
        bits, _, _ = _readout(kind, s, p, at, causal, keep=keep)
        differing = np.argwhere((m != true) & vis[None, None])
        got = MR.wrong_bits(bits, want)
        print(f"[readout-mutant] {kind} causal {causal} {name}: {len(got)} wrong bits decoded, {len(differing)} planted")
        assert len(differing) > 0 and np.array_equal(got, differing), name
        with pytest.raises(AssertionError) as e:
            MR.compare(bits, want, at, name)
        text = str(e.value)
        assert f"{len(differing)} wrong mask bits" in text
        for b, h, i, j in differing[:10]:                                  # global coordinates and the lane group
            assert f"({b}, {h + at[2]}, {i + at[0]}, {j + at[1]}) [tile {j // 64}, row%32 {i % 32}, key%4 {j % 4}]" in text, text
        assert text.count("[tile") == min(10, len(differing))


def test_decoder_refuses_what_is_no_integer():
    s, p = SHAPES[0], 0.5
    passes = MR.build("dv", s, p)
    res = _solve("dv", s, p, passes, (0, 0, 0), False, None, 0)
    res[0][1, 7, 1, 3] += 0.25 * 2.0                                       # x = dv t/256: a quarter off
    with pytest.raises(AssertionError, match="from an integer"):
        MR.decode("dv", s, p, passes, res)
    # a dQ pass of 8 planes at t = 230 is not built; a power-of-two threshold lifts the limit
    assert (MR.plane_cap("dq", "bfloat16", 0.1), MR.plane_cap("dq", "float16", 0.1), MR.plane_cap("dq", "bfloat16", 0.75)) == (4, 6, 16)
