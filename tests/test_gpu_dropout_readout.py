"""The dropout kernels' keep mask, read out bit for bit (tests/mask_readout.py): with q = 0, lse = 0, delta = 0 and bit-plane
operands the forward, dQ, dK and dV of usp_flash_fwd_dropout / usp_flash_bwd_dropout print `keep & visible` as exact integers.
Expected everywhere: dropout_ref.keep_mask(p, seed, ..., row0, key0, head0) & shift_ref.visible(...), compared for EVERY
(batch, head, row, key) -- ragged ends (Sq % 4 = 3, Sk % 4 = 2), K splits and cuts of 2 and 3, every dkdv_heads, windows and
shifts that are no multiple of 4, both forward workgroup shapes, merge_in, more work items than CUs, the thresholds t = 1 and
t = 255 the tolerance tests cannot look at, and offsets at the edge of what the entry points serve (NEAR).  A mismatch names
(batch, head, global row, global key), the key tile, row mod 32 and key mod 4.  Every case asserts the launch kinds and prints a
[readout] line: kinds, bits compared, largest |x - rint(x)| (profiles/mask_readout.txt quotes them)."""
import numpy as np
import pytest
import torch

import dropout_ref
import mask_readout as MR
from shift_ref import visible
from test_gpu_dropout import FAR

pytestmark = pytest.mark.gpu

SEED = (1 << 40) + 1234                    # above 2^32: both key words matter
PROBS = tuple(MR.PROBS)
_WAVE_FWD = {"fwd_wave8", "fwd_wave4", "fwd_split_merge"}
_WAVE_BWD = {"dkdv_wave8", "dq_wave8", "reduce_heads", "reduce_cuts"}


def near(s):
    """The largest multiples of 4 with row0 + Sq < 2^31 and key0 + Sk < 2^31, head0 = 7: one step below what is declined."""
    return (((1 << 31) - 1 - s.Sq) // 4 * 4, ((1 << 31) - 1 - s.Sk) // 4 * 4, 7)


def offsets(s):
    return ((0, 0, 0), FAR, near(s))


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


_PASSES = {}


def _passes(dev, kind, s, p, **kw):
    """The builder's passes on the device; they depend on p only through the number of planes a pass may hold."""
    key = (kind, s, MR.plane_cap(kind, s.dt, p, **kw))
    if key not in _PASSES:
        while len(_PASSES) >= 8:
            _PASSES.pop(next(iter(_PASSES)))
        _PASSES[key] = [MR.Pass(*(None if t is None else t.to(dev) for t in ps[:4]), ps.planes, ps.lo) for ps in MR.build(kind, s, p, **kw)]
    return _PASSES[key]


def _want(s, p, at, causal, window=None, shift=0):
    """keep & visible; the bytes are generated once per (shape, offsets) and reused across p."""
    by = dropout_ref.keep_bytes(SEED, s.B, s.Hq, s.Sq, s.Sk, *at)
    vis = visible(s.Sq, s.Sk, causal, window, shift or 0).numpy()
    return (by < dropout_ref.threshold(p)) & vis[None, None], vis          # (t <= 255 for every p used here)


def _note(what, kinds, n, dev_):
    print(f"[readout] {what}: kinds {'+'.join(kinds)} bits {n} max|x-rint(x)| {dev_:.2e}")


def read_fwd(dev, s, p, at, causal, what, kinds_ok, window=None, shift=None, out16=False, merged=False, want_at=None, **kw):
    """One forward read-out (all passes), decoded from the fp32 `acc` (final_end = 0) or, with out16, from the 16-bit `out`.
    `want_at`: the offsets of the expected mask where they are not the call's (the negative control)."""
    from yunchang_amd import _C
    res = []
    for ps in _passes(dev, "fwd", s, p, merged=merged, out16=out16):
        lse = torch.full((s.B, s.Hq, s.Sq), float("nan"), dtype=torch.float32, device=dev)
        if out16:
            dst = torch.full_like(ps.q, float("nan"))
            _C.flash_fwd(ps.q, ps.k, ps.v, MR.SCALE, causal, lse, out=dst, window=window, shift=shift, dropout=(p, SEED) + at, **kw)
        else:
            dst = torch.full(ps.q.shape, float("nan"), dtype=torch.float32, device=dev)
            _C.flash_fwd(ps.q, ps.k, ps.v, MR.SCALE, causal, lse, acc=dst, final_end=0, window=window, shift=shift,
                         dropout=(p, SEED) + at, **kw)
        kinds = _C.last_launch_kinds()
        assert kinds_ok(kinds), (what, kinds)
        res.append(dst)
    want, vis = _want(s, p, at if want_at is None else want_at, causal, window, shift)
    bits, worst = MR.decode("fwd", s, p, _passes(dev, "fwd", s, p, merged=merged, out16=out16), res, vis)
    n = MR.compare(bits, want, at, what)
    _note(what, kinds, n, worst)
    return kinds


def read_bwd(dev, kind, s, p, at, causal, what, kinds_ok, window=None, shift=None, want_at=None, **kw):
    """One backward read-out: dq, dk or dv carries the bits, the outputs the problem makes exactly zero are checked to be."""
    from yunchang_amd import _C
    lse, delta = MR.stats(s, dev)
    res = []
    passes = _passes(dev, kind, s, p)
    for ps in passes:
        dq, dk, dv = (torch.full(t.shape, float("nan"), dtype=torch.float32, device=dev) for t in (ps.q, ps.k, ps.v))
        _C.flash_bwd(ps.dout, ps.q, ps.k, ps.v, lse, delta, dq, dk, dv, MR.SCALE, causal, window=window, shift=shift,
                     dropout=(p, SEED) + at, **kw)
        kinds = _C.last_launch_kinds()
        assert kinds_ok(kinds), (what, kinds)
        for name, z in {"dq": (("dk", dk),), "dk": (("dq", dq),), "dv": (("dq", dq), ("dk", dk))}[kind]:
            assert bool((z == 0).all()), f"{what}: {name} must be exactly 0"
        res.append({"dq": dq, "dk": dk, "dv": dv}[kind])
    want, _ = _want(s, p, at if want_at is None else want_at, causal, window, shift)
    bits, worst = MR.decode(kind, s, p, passes, res)
    n = MR.compare(bits, want, at, what)
    _note(what, kinds, n, worst)
    return kinds


def _bwd_kinds(s, splits, heads):
    """The kinds a backward call must launch: a reduce over cuts iff dQ is cut, one over heads iff dK/dV has more than one slab."""
    want = {"dkdv_wave8", "dq_wave8"} | ({"reduce_cuts"} if splits[0] > 1 else set())
    if heads:
        return lambda k: set(k) == want | ({"reduce_heads"} if (s.Hq // s.Hkv // heads) * max(1, splits[1]) > 1 else set())
    return lambda k: want <= set(k) <= want | {"reduce_heads"}


# ---- 1. block cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("causal", [True, False])
def test_block_forward(dev, causal, D, dt):
    """Every p at each of (k_splits, interleave); the offsets rotate, so that every p meets every offset in a parameter set."""
    s = MR.Shape(2, 203, 8 * D - 2, 4, 2, D, dt)
    for vi, (ks, il) in enumerate(((0, False), (0, True), (3, False), (3, True))):
        ok = (lambda k: k == ("fwd_wave4",)) if ks == 0 else (lambda k: set(k) == {"fwd_wave4", "fwd_split_merge"})
        for pi, p in enumerate(PROBS):
            at = offsets(s)[(vi + pi) % 3]
            read_fwd(dev, s, p, at, causal, f"fwd D{D} {dt} causal {causal} k_splits {ks} interleave {il} p {p:.4f} at {at}", ok,
                     merged=ks > 0, k_splits=ks, interleave=il)


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("causal", [True, False])
def test_block_backward(dev, causal, D, dt):
    """dQ, dK and dV at every (splits, dkdv_heads); p and the offsets rotate.  Sq = 515 (D 64, D 128): more than one 256-row dQ
    block and several 128-key dK/dV blocks, ragged; there one read-out per (splits, dkdv_heads), the kind in rotation."""
    rot = D // 32 + (dt == "float16") + causal
    for Sq in (203, 515) if D >= 64 else (203,):
        s = MR.Shape(2, Sq, 8 * D - 2, 4, 2, D, dt)
        for j, (splits, heads) in enumerate((c, h) for c in ((0, 0), (2, 2), (3, 3)) for h in (0, 1, 2)):
            for c, kind in enumerate(("dq", "dk", "dv")):
                if Sq == 515 and (j + rot) % 3 != c:
                    continue
                p, at = PROBS[(j + 2 * c + rot) % 6], offsets(s)[(j + c) % 3]      # every kind meets every p and every offset
                read_bwd(dev, kind, s, p, at, causal,
                         f"{kind} D{D} {dt} causal {causal} Sq {Sq} splits {splits} dkdv_heads {heads} p {p:.4f} at {at}",
                         _bwd_kinds(s, splits, heads), splits=splits, dkdv_heads=heads)


# ---- 2. window and shift -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dt", [(128, "bfloat16"), (64, "float16")])
@pytest.mark.parametrize("causal,window,shift", [(True, (70, 0), None), (False, (100, 40), None), (True, None, -37), (True, None, 64)])
def test_window_and_shift(dev, causal, window, shift, D, dt):
    """The left bound is the only path that moves t_begin / t0 under a K cut: every read-out plain and cut."""
    s = MR.Shape(2, 203, 8 * D - 2, 4, 2, D, dt)
    tag = f"D{D} {dt} causal {causal} window {window} shift {shift}"
    for i, (ks, splits) in enumerate(((0, (0, 0)), (3, (3, 2)))):
        p, at = (0.1, 0.9)[i], offsets(s)[1 + i]
        read_fwd(dev, s, p, at, causal, f"fwd {tag} k_splits {ks} p {p}", lambda k: set(k) <= _WAVE_FWD and ("fwd_split_merge" in k) == (ks > 0),
                 window, shift, merged=ks > 0, k_splits=ks)
        for kind in ("dq", "dk", "dv"):
            read_bwd(dev, kind, s, p, at, causal, f"{kind} {tag} splits {splits} p {p}", _bwd_kinds(s, splits, 1), window, shift,
                     splits=splits, dkdv_heads=1)


# ---- 3. the 8-wave forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Sk,dt,p,causal", [(128, 509, "bfloat16", 0.1, True), (32, 254, "float16", 255.0 / 256, False)])
def test_eight_wave_forward(dev, D, Sk, dt, p, causal):
    """256-row workgroups (launch_fwd: 320 items of 256 rows, a causal launch of more than 1024 rows).  The causal case shifts the
    diagonal to the top-left corner (Sq > Sk: bottom-right alignment would leave the first 591 rows without a key), so every
    query tile has a diagonal tile or a full row of keys."""
    s = MR.Shape(2, 1100, Sk, 32, 8, D, dt)
    at, shift = (near(s), s.Sq - s.Sk) if causal else (FAR, None)
    what = f"8 waves D{D} {dt} causal {causal} shift {shift} p {p:.4f}"
    read_fwd(dev, s, p, at, causal, what, lambda k: k == ("fwd_wave8",), shift=shift, k_splits=0)
    read_fwd(dev, s, p, at, causal, f"{what} k_splits 2", lambda k: set(k) == {"fwd_wave8", "fwd_split_merge"}, shift=shift,
             merged=True, k_splits=2)


# ---- 4. merge_in: two key runs forming one ring row --------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dt,p", [(64, "bfloat16", 0.1), (32, "float16", 0.75)])
def test_merge_in(dev, D, dt, p):
    """The second call's key0 is advanced by the first run's length h (a multiple of 4, not of 64); rows [50, 150) are final:
    decoded from the 16-bit `out` (4 planes a pass), the others from `acc`."""
    from yunchang_amd import _C
    s = MR.Shape(2, 203, 8 * D - 2, 4, 2, D, dt)
    h, at = 2 * D + 36, FAR
    assert h % 4 == 0 and h % 64 != 0
    passes = _passes(dev, "fwd", s, p, out16=True)
    accs, outs = [], []
    for ps in passes:
        acc = torch.full(ps.q.shape, float("nan"), dtype=torch.float32, device=dev)
        out = torch.full_like(ps.q, float("nan"))
        lse = torch.full((s.B, s.Hq, s.Sq), float("nan"), dtype=torch.float32, device=dev)
        _C.flash_fwd(ps.q, ps.k[:, :h], ps.v[:, :h], MR.SCALE, False, lse, out=out, acc=acc, final_end=0, k_splits=0,
                     dropout=(p, SEED) + at)
        k1 = _C.last_launch_kinds()
        _C.flash_fwd(ps.q, ps.k[:, h:], ps.v[:, h:], MR.SCALE, False, lse, out=out, acc=acc, merge_in=True, final_begin=50, final_end=150,
                     k_splits=0, dropout=(p, SEED, at[0], at[1] + h, at[2]))
        kinds = _C.last_launch_kinds()
        assert k1 == kinds == ("fwd_wave4",), (k1, kinds)
        assert bool(torch.isfinite(lse).all())
        accs.append(acc)
        outs.append(out)
    want, vis = _want(s, p, at, False)
    final = np.zeros(s.Sq, dtype=bool)
    final[50:150] = True
    b_out, d_out = MR.decode("fwd", s, p, passes, outs, vis, rows=slice(50, 150))
    b_acc0, d0 = MR.decode("fwd", s, p, passes, accs, vis, rows=slice(0, 50))
    b_acc1, d1 = MR.decode("fwd", s, p, passes, accs, vis, rows=slice(150, s.Sq))
    n = MR.compare(b_out | b_acc0 | b_acc1, want, at, f"merge_in D{D} {dt} p {p}")
    _note(f"merge_in D{D} {dt} p {p} h {h}: out rows [50, 150) dev {d_out:.2e}, acc rows", kinds, n, max(d0, d1))


# ---- 5. more work items than CUs -----------------------------------------------------------------------------------------------------------
def test_more_items_than_cus(dev):
    """A persistent multi-pass walk of every kernel; the causal forward takes the 4-wave workgroups, the full one the 8-wave ones."""
    Bc, S, Hq, Hkv, D, dt, p = 5, 512, 32, 8, 64, "bfloat16", 0.5
    s = MR.Shape(Bc, S, S, Hq, Hkv, D, dt)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    at = (8, 4, 3)
    for causal in (True, False):
        fwd_items = Bc * Hq * ((S + 127) // 128 if causal else (S + 255) // 256)
        assert fwd_items > cus * (2 if causal else 1) and Bc * Hq * ((S + 255) // 256) > cus and Bc * Hkv * ((S + 127) // 128) * 2 > cus
        what = f"B{Bc} H{Hq}/{Hkv} S{S} causal {causal}"
        read_fwd(dev, s, p, at, causal, f"fwd {what}", lambda k: k == (("fwd_wave4",) if causal else ("fwd_wave8",)), k_splits=0)
        read_bwd(dev, "dq", s, p, at, causal, f"dq {what}", lambda k: {"dkdv_wave8", "dq_wave8"} <= set(k) <= _WAVE_BWD)
        for i, heads in enumerate((0, 2, 4)):                 # dK and dV leave one launch with one mask: they alternate
            kind = ("dk", "dv")[(i + causal) % 2]
            read_bwd(dev, kind, s, p, at, causal, f"{kind} {what} dkdv_heads {heads}", _bwd_kinds(s, (0, 0), heads), splits=(0, 0),
                     dkdv_heads=heads)


# ---- 6. the 16-bit `out` -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dt,p,causal", [(128, "bfloat16", 0.9, True), (64, "float16", 1.0 / 256, False)])
def test_sixteen_bit_out(dev, D, dt, p, causal):
    s = MR.Shape(2, 203, 8 * D - 2, 4, 2, D, dt)
    read_fwd(dev, s, p, near(s), causal, f"16-bit out D{D} {dt} causal {causal} p {p:.4f}", lambda k: k == ("fwd_wave4",), out16=True,
             k_splits=0)


# ---- 7. the comparison can fail ------------------------------------------------------------------------------------------------------------
def test_another_position_is_seen(dev):
    """The kernels at one patch further down, across or one head further than the expected mask: about half of the bits differ
    (p = 0.5) and the report counts them.  (That the decoder localises single bits is shown without a GPU in
    tests/test_mask_readout_cpu.py.)"""
    s, p = MR.Shape(2, 203, 254, 4, 2, 32, "bfloat16"), 0.5
    ok = lambda k: bool(k)
    for i, at in enumerate(((4, 0, 0), (0, 4, 0), (0, 0, 1))):
        for kind in MR.KINDS:
            with pytest.raises(AssertionError, match=r"\d{5,} wrong mask bits"):
                if kind == "fwd":
                    read_fwd(dev, s, p, at, bool(i % 2), f"control fwd at {at}", ok, want_at=(0, 0, 0), k_splits=0)
                else:
                    read_bwd(dev, kind, s, p, at, bool(i % 2), f"control {kind} at {at}", ok, want_at=(0, 0, 0))
