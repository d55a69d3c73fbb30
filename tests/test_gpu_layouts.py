"""Every kernel of the C ABI with an independent memory layout for each tensor of the call (tests/layout_util.py).

include/usp_hip.h gives every tensor its own pointer and stride triple; the other GPU tests build contiguous tensors, so
K and V (dK / dV, q / dout, out / acc, lse / delta) always share their strides there.  Each cell below is a seeded sweep of
small ragged shapes in which every tensor draws its layout independently; a case runs once contiguous and once strided with
the kernel family pinned, asserts which kernels ran, and requires bit-identical results, the contiguous run inside the stated
tolerances of the fp64 oracle, an intact arena around every view and the header's "not touched" promises.

No case of a sweep is skipped or refused: each generator draws only what its kernels serve; what the library refuses has its
own test (`test_row64_stride_conditions_*`, `test_wave8_dkdv_32bit_offset_bound`).  The last test of the file reports, per
cell, how many cases were drawn and compared and which launch kinds ran strided, and requires every USP_KIND_* bit among them.

USP_LAYOUT_CASES=n sets the seeds per cell (default 8: the GPU suite has a time bar, tests/conftest.py).
"""
import os

import numpy as np
import pytest
import torch

import layout_util as LU
from golden_util import TOL, assert_close
from oracle import usp_oracle as O

pytestmark = pytest.mark.gpu

N_CELL = int(os.environ.get("USP_LAYOUT_CASES", "8"))
ALL_KINDS = ("fwd_row64", "fwd_wave8", "fwd_wave4", "fwd_split_merge", "dkdv_row64", "dkdv_wave8", "dq_row64", "dq_wave8",
             "reduce_heads", "reduce_cuts")
REPORT = {}                                                  # cell -> dict(drawn=, compared=, kinds=set())


@pytest.fixture(scope="module")
def dev():
    from yunchang_amd import _C
    _C.load()
    return torch.device("cuda:0")


class HipOps:
    """The runner's `ops` seam over the ctypes binding."""

    def fwd(self, q, k, v, scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None, k_splits=0,
            window=None, softcap=None, family=None):
        from yunchang_amd import _C
        _C.flash_fwd(q, k, v, scale, causal, lse, out=out, acc=acc, merge_in=merge_in, final_begin=final_begin,
                     final_end=final_end, k_splits=k_splits, window=window, family=family, softcap=softcap)

    def delta(self, dout, out, delta):
        from yunchang_amd import _C
        _C.bwd_delta(dout, out, delta)

    def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, scale, causal, accum_dq=False, accum_dk=False, accum_dv=False,
            dq16=None, dk16=None, dv16=None, window=None, softcap=None, family=None, only=None, splits=(0, 0), dkdv_heads=0):
        from yunchang_amd import _C
        _C.flash_bwd(dout, q, k, v, lse, delta, dq, dk, dv, scale, causal, accum_dq=accum_dq, accum_dk=accum_dk,
                     accum_dv=accum_dv, dq16=dq16, dk16=dk16, dv16=dv16, splits=splits, window=window, family=family, only=only,
                     dkdv_heads=dkdv_heads, softcap=softcap)

    def fwd_packed(self, q, k, v, seq_q, seq_k, max_q, max_k, scale, causal, lse, out=None, sched=True, softcap=None):
        from yunchang_amd import _C
        _C.flash_fwd_packed(q, k, v, seq_q, seq_k, max_q, max_k, scale, causal, lse, out=out, sched=sched, softcap=softcap)
        assert _C.last_launch_kinds() in (("fwd_wave8",), ("fwd_wave4",)), _C.last_launch_kinds()
        self.packed_kinds = set(_C.last_launch_kinds())

    def bwd_packed(self, dout, q, k, v, lse, delta, seq_q, seq_k, max_q, max_k, dq, dk, dv, scale, causal, accum_dq=False,
                   accum_dk=False, accum_dv=False, dq16=None, dk16=None, dv16=None, sched=True, softcap=None):
        from yunchang_amd import _C
        _C.flash_bwd_packed(dout, q, k, v, lse, delta, seq_q, seq_k, max_q, max_k, dq, dk, dv, scale, causal, accum_dq=accum_dq,
                            accum_dk=accum_dk, accum_dv=accum_dv, dq16=dq16, dk16=dk16, dv16=dv16, sched=sched, softcap=softcap)
        kinds = set(_C.last_launch_kinds())               # packed batches: the 8-wave kernels, one query head per dK/dV item
        assert kinds == {"dkdv_wave8", "dq_wave8"} | ({"reduce_heads"} if q.shape[1] > k.shape[1] else set()), kinds
        self.packed_kinds |= kinds
        assert int(_C.sched_block(q.device).abs().sum()) == 0, "the work-queue control block must be left zeroed"

    def kinds(self):
        from yunchang_amd import _C
        torch.cuda.synchronize()
        return _C.last_launch_kinds()


# ---- case generators ---------------------------------------------------------------------------------------------------------
def _shape(rs, D=None, rows=400):
    D = int(rs.choice([32, 64, 128])) if D is None else D
    dt = str(rs.choice(["bfloat16", "float16"]))
    Hkv = int(rs.choice([1, 2, 3]))
    Hq = Hkv * int(rs.choice([1, 2, 4]))
    B = int(rs.choice([1, 2, 3]))
    Sq = int(rs.randint(1, rows))
    Sk = Sq if rs.rand() < 0.4 else int(rs.randint(1, rows))
    return B, Sq, Sk, Hq, Hkv, D, bool(rs.rand() < 0.6), dt


def _variant(rs, i):
    """Every third case a sliding window, every third a softcap (wave32 family only)."""
    if i % 3 == 1:
        return dict(window=(int(rs.choice([0, 17, 64, 200])), int(rs.choice([-1, 0, 3, 40]))))
    if i % 3 == 2:
        return dict(softcap=float(rs.choice([2.5, 6.0])))
    return {}


def _fwd_wave_kind(c):
    """The workgroup shape launch_fwd picks inside the 32-rows-per-wave family (usp_flash_fwd.hip)."""
    grid8 = c.B * c.Hq * ((c.Sq + 255) // 256) * max(1, c.k_splits)
    tri = c.causal or (c.window is not None and c.window[1] >= 0)
    return "fwd_wave4" if (grid8 < 256 or (tri and c.Sq <= 1024)) else "fwd_wave8"


def case_fwd_wave4(rs, i):
    c = LU.Case(*_shape(rs), family="wave32", **_variant(rs, i))
    c.kinds = {_fwd_wave_kind(c)}
    return c


def case_fwd_wave8(rs, i):
    """256 items of 256 rows: the 8-wave shape.  Many rows, few keys: the oracle stays cheap."""
    dt = str(rs.choice(["bfloat16", "float16"]))
    Hkv = int(rs.choice([4, 8, 16]))
    c = LU.Case(2, int(rs.randint(1793, 2048)), int(rs.randint(1, 130)), 16, Hkv, int(rs.choice([32, 64, 128])), bool(i % 2), dt,
                family="wave32", **_variant(rs, i))
    c.kinds = {_fwd_wave_kind(c)}
    assert c.kinds == {"fwd_wave8"}
    return c


def case_fwd_row64(rs, i):
    return LU.Case(*_shape(rs, 128, 600), family="row64", ss128=("k",), kinds={"fwd_row64"})


def _ring(rs, Sq, Sk):
    Sa = int(rs.randint(1, Sk)) if Sk > 1 else 0
    fb = int(rs.randint(0, Sq))
    return Sa, fb, int(rs.randint(fb, Sq + 1))


def case_fwd_ring(rs, i):
    fam = ("wave32", "row64")[i % 2]
    B, Sq, Sk, Hq, Hkv, D, causal, dt = _shape(rs, 128 if fam == "row64" else None)
    Sk += 1                                                  # two calls: at least one key each
    ks = int(rs.choice([0, 0, 2, 3]))
    c = LU.Case(B, Sq, Sk, Hq, Hkv, D, causal, dt, family=fam, ring=_ring(rs, Sq, Sk), k_splits=ks,
                ss128=("k",) if fam == "row64" else ())
    c.kinds = {"fwd_row64" if fam == "row64" else _fwd_wave_kind(c)} | ({"fwd_split_merge"} if ks > 1 else set())
    return c


def case_fwd_ksplit(rs, i):
    fam = ("wave32", "row64")[i % 2]
    ks = int(rs.choice([2, 3, 4, 5, 8]))
    c = LU.Case(*_shape(rs, 128 if fam == "row64" else int(rs.choice([64, 128])), 700), family=fam, k_splits=ks,
                ss128=("k",) if fam == "row64" else ())
    c.kinds = {"fwd_row64" if fam == "row64" else _fwd_wave_kind(c), "fwd_split_merge"}
    return c


FORMS = ("f32", "f32+", "h16", "h16+")


def _bwd_kinds(c, fam):
    G = c.Hq // c.Hkv
    k = set()
    if c.only != "dq":
        k.add("dkdv_row64" if fam == "row64" else "dkdv_wave8")
        if (G // (c.dkdv_heads or G)) * max(1, c.splits[1]) > 1:
            k.add("reduce_heads")
    if c.only != "dkdv":
        k.add("dq_row64" if fam == "row64" else "dq_wave8")
        if c.splits[0] > 1:
            k.add("reduce_cuts")
    return k


def _bwd_case(rs, i, fam, cuts):
    B, Sq, Sk, Hq, Hkv, D, causal, dt = _shape(rs, 128 if fam == "row64" else None)
    if cuts and Hq == Hkv:
        Hq = Hkv * 2
    G = Hq // Hkv
    forms = tuple(str(rs.choice(FORMS)) for _ in range(3))
    only = [None, None, None, "dq", "dkdv"][rs.randint(5)]
    splits = (int(rs.choice([0, 2, 3, 8])), int(rs.choice([0, 2, 4]))) if cuts else (0, 0)
    heads = int(rs.choice([1, G])) if cuts else G
    var = _variant(rs, i) if fam == "wave32" and not cuts else {}
    c = LU.Case(B, Sq, Sk, Hq, Hkv, D, causal, dt, family=fam, forms=forms, only=only, splits=splits, dkdv_heads=heads,
                ss128=("q", "dout", "k", "v") if fam == "row64" else (), **var)
    c.kinds = _bwd_kinds(c, fam)
    return c


CELLS = {
    # name: (call, generator)
    "fwd wave32 4-wave": ("fwd", case_fwd_wave4),
    "fwd wave32 8-wave": ("fwd", case_fwd_wave8),
    "fwd row64": ("fwd", case_fwd_row64),
    "fwd ring step": ("fwd", case_fwd_ring),
    "fwd K split": ("fwd", case_fwd_ksplit),
    "bwd wave32": ("bwd", lambda rs, i: _bwd_case(rs, i, "wave32", False)),
    "bwd row64": ("bwd", lambda rs, i: _bwd_case(rs, i, "row64", False)),
    "bwd GQA / cuts wave32": ("bwd", lambda rs, i: _bwd_case(rs, i, "wave32", True)),
    "bwd GQA / cuts row64": ("bwd", lambda rs, i: _bwd_case(rs, i, "row64", True)),
    "delta": ("delta", lambda rs, i: LU.Case(*_shape(rs))),
}
N_OF = {"fwd wave32 8-wave": max(2, N_CELL // 2)}            # the one cell with thousands of rows per case
CHECK = {"fwd": LU.check_fwd_case, "bwd": LU.check_bwd_case, "delta": LU.check_delta_case}
SWEEP = [(name, i) for name in CELLS for i in range(N_OF.get(name, N_CELL))]
# the seed of a case = its number among the cases of the same call (layout_util.draw_layouts walks the layout kinds by it)
SEED = {}
for _n, _i in SWEEP:
    SEED[(_n, _i)] = sum(1 for k in SEED if CELLS[k[0]][0] == CELLS[_n][0])


def sweep_cases(call):
    """(cell, seed, case) of every case of the sweep for `call` -- pure host code, so the CPU self-test can look at it."""
    return [(n, SEED[(n, i)], CELLS[n][1](np.random.RandomState(40000 + 1000 * list(CELLS).index(n) + i), i))
            for n, i in SWEEP if CELLS[n][0] == call]


def _note(cell, kinds, drawn=1, compared=1):
    r = REPORT.setdefault(cell, dict(drawn=0, compared=0, kinds=set()))
    r["drawn"] += drawn
    r["compared"] += compared
    for k in kinds or ():
        r["kinds"] |= set(k) if isinstance(k, (tuple, list, set)) else {k}


@pytest.mark.parametrize("cell,i", SWEEP, ids=[f"{n.replace(' ', '_')}-{i}" for n, i in SWEEP])
def test_layout_sweep(dev, cell, i):
    call = CELLS[cell][0]
    _, seed, case = next(t for t in sweep_cases(call) if t[0] == cell and t[1] == SEED[(cell, i)])
    _note(cell, (), 1, 0)
    kinds = CHECK[call](HipOps(), case, seed, dev)
    _note(cell, kinds if call == "fwd" else [kinds or ()], 0, 1)


@pytest.mark.parametrize("i", range(N_CELL))
def test_packed_layout_sweep(dev, i):
    """Packed forward and backward: token tensors with their own stride_s / stride_h, (H,T) row statistics with stride_h > T,
    the dynamic item queue on (even i) and off; rows outside every sequence stay untouched."""
    pc = LU.draw_packed_case(np.random.RandomState(41000 + i), i)
    if i % 3 == 2:
        pc.softcap = 6.0
    _note("packed fwd + bwd", (), 1, 0)
    ops = HipOps()
    LU.check_packed_case(ops, pc, i, dev)
    _note("packed fwd + bwd", [ops.packed_kinds], 0, 1)


# ---- usp_lse_merge -------------------------------------------------------------------------------------------------------------
def _run_merge(dev, B, S, H, D, dt, first, seed, layouts):
    from yunchang_amd import _C
    rs = np.random.RandomState(seed)
    acc = rs.standard_normal((B, S, H, D)).astype(np.float32)
    bo = LU.round_to(rs.standard_normal((B, S, H, D)).astype(np.float32), dt)
    lse, bl = (rs.standard_normal((B, H, S)).astype(np.float32) * 3 for _ in range(2))
    # rows without a visible key so far / in the block / in both: lse = -inf and a zero output row, as the kernels emit them
    for i, (l_, o_) in enumerate(((lse, acc), (bl, bo), (None, None))):
        rows = rs.rand(B, H, S) < 0.08
        for l2, o2 in ((l_, o_),) if l_ is not None else ((lse, acc), (bl, bo)):
            l2[rows] = -np.inf
            o2[np.swapaxes(rows, 1, 2)] = 0.0
    ar = LU.Arena(dev)
    t_acc = LU.place(torch.from_numpy(acc).to(dev), layouts["acc"], ar, "acc", track=False)
    t_lse = LU.place(torch.from_numpy(lse).to(dev), layouts["lse"], ar, "lse", track=False)
    t_bo = LU.place(LU._tt(bo, dt, dev), layouts["blk_out"], ar, "blk_out")
    t_bl = LU.place(torch.from_numpy(bl).to(dev), layouts["blk_lse"], ar, "blk_lse")
    _C.lse_merge(t_acc, t_lse, t_bo, t_bl, first)
    torch.cuda.synchronize()
    bad = ar.violations()
    assert not bad, f"merge: written outside the views: {bad}"
    assert ar.unchanged(), "merge: the block's tensors were modified"
    return dict(acc=LU._host(t_acc), lse=LU._host(t_lse), inputs=(acc, lse, bo, bl))


MERGE_TENSORS = ("acc", "lse", "blk_out", "blk_lse")


@pytest.mark.parametrize("i", range(2 * N_CELL))
def test_lse_merge_layouts(dev, i):
    rs = np.random.RandomState(41100 + i)
    B, S, _, H, _, D, _, dt = _shape(rs)
    first = bool(i % 3 == 0)
    case = LU.Case(B, S, S, H, H, D, False, dt)
    layouts = LU.draw_layouts(np.random.RandomState(93000 + i), case, MERGE_TENSORS, i)
    what = f"merge B{B} S{S} H{H} D{D} {dt} first={first} layouts {layouts}"
    _note("usp_lse_merge", (), 1, 0)
    base = _run_merge(dev, B, S, H, D, dt, first, i, LU.contiguous_layouts(MERGE_TENSORS))
    got = _run_merge(dev, B, S, H, D, dt, first, i, layouts)
    acc, lse, bo, bl = base["inputs"]
    if first:
        ro, rl = bo.astype(np.float64), bl.astype(np.float64)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            ro, l4 = O.update_out_and_lse(acc.astype(np.float64), np.swapaxes(lse, 1, 2)[..., None].astype(np.float64), bo, bl)
        rl = np.swapaxes(l4[..., 0], 1, 2)
        # a running row without any key so far adopts the block (the oracle's `lse - logsigmoid(lse - blk)` is -inf + inf there)
        rl = np.where(np.isneginf(lse), bl, rl)
    assert_close(base["lse"].numpy(), rl, 1e-5, 1e-5, what + " lse")
    assert_close(base["acc"].numpy(), ro, 1e-5, 1e-5, what + " acc")
    LU.assert_same_bits(base["acc"], got["acc"], what + ": acc")
    LU.assert_same_bits(base["lse"], got["lse"], what + ": lse")
    _note("usp_lse_merge", (), 0, 1)


# ---- copy / sum / cast / add ---------------------------------------------------------------------------------------------------
def _gapped(rs, dev, dtype, sizes, row, align):
    """A sentinel-filled buffer and the element strides of a 4-level nest of `sizes` rows of `row` elements with a gap of
    its own behind every level (multiples of `align` elements) and guard bands on both sides."""
    strides, span = [], row
    for n in reversed(sizes):
        span += align * int(rs.randint(0, 4))
        strides.append(span)
        span *= n
    strides = strides[::-1]
    front = align * int(rs.randint(1, 9)) + 1024
    raw = torch.full((front + span + 1024,), LU.SENTINEL[dtype], dtype=LU._RAW[dtype], device=dev)
    buf = raw.view(dtype)
    view = buf.as_strided(tuple(sizes) + (row,), tuple(strides) + (1,), front)
    owned = torch.zeros(raw.shape, dtype=torch.bool, device=dev)
    owned.as_strided(view.shape, view.stride(), front).fill_(True)
    return raw, owned, view, strides


def _outside_intact(raw, owned, dtype):
    return not bool(((raw != LU.SENTINEL[dtype]) & ~owned).any())


@pytest.mark.parametrize("i", range(N_CELL))
def test_copy_and_sum_rows_with_gaps_on_both_sides(dev, i):
    from yunchang_amd import _C
    rs = np.random.RandomState(41200 + i)
    dtype = (torch.bfloat16, torch.float16)[i % 2]
    sizes = [int(rs.randint(1, 5)) for _ in range(4)]
    row = 8 * int(rs.randint(1, 40))
    sraw, sown, src, ss = _gapped(rs, dev, dtype, sizes, row, 8)
    draw, down, dst, ds = _gapped(rs, dev, dtype, sizes, row, 8)
    src.copy_(torch.randn(src.shape, device=dev).to(dtype))
    keep = LU.raw_bits(src).clone()
    _C.copy_rows(dst, src, row * 2, sizes, [s * 2 for s in ds], [s * 2 for s in ss])
    torch.cuda.synchronize()
    assert torch.equal(LU.raw_bits(dst), keep) and torch.equal(LU.raw_bits(src), keep)
    assert _outside_intact(draw, down, dtype) and _outside_intact(sraw, sown, dtype)
    # r-term sum: the terms are the outermost level of the source
    r = sizes[0]
    draw, down, dst, ds = _gapped(rs, dev, dtype, sizes[1:], row, 8)
    _C.sum_rows(dst, src, row * 2, r, ss[0] * 2, sizes[1:], [s * 2 for s in ds], [s * 2 for s in ss[1:]])
    torch.cuda.synchronize()
    want = torch.zeros(dst.shape, dtype=torch.float32, device=dev)
    for t in range(r):
        want = want + src[t].float()                          # fp32, ascending t, rounded once
    assert torch.equal(LU.raw_bits(dst), LU.raw_bits(want.to(dtype)))
    assert _outside_intact(draw, down, dtype) and torch.equal(LU.raw_bits(src), keep)
    _note("copy / sum", (), 1, 1)


@pytest.mark.parametrize("i", range(N_CELL))
def test_cast_and_add_row_strides_and_aliasing(dev, i):
    from yunchang_amd import _C
    rs = np.random.RandomState(41300 + i)
    dtype = (torch.bfloat16, torch.float16)[i % 2]
    B, n = int(rs.randint(2, 5)), 8 * int(rs.randint(1, 300))
    shape4 = (B, 1, 1, n)

    def rows(dt, align):
        gap = align * int(rs.randint(0, 5))
        front = align * int(rs.randint(1, 9)) + 1024
        raw = torch.full((front + B * (n + gap) + 1024,), LU.SENTINEL[dt], dtype=LU._RAW[dt], device=dev)
        view = raw.view(dt).as_strided(shape4, (n + gap, n, n, 1), front)
        owned = torch.zeros(raw.shape, dtype=torch.bool, device=dev)
        owned.as_strided(shape4, view.stride(), front).fill_(True)
        return raw, owned, view

    araw, aown, a = rows(torch.float32, 4)
    braw, bown, b = rows(torch.float32, 4)
    a.copy_(torch.randn(shape4, device=dev))
    b.copy_(torch.randn(shape4, device=dev))
    a0, b0 = a.clone(), b.clone()
    draw, down, d16 = rows(dtype, 8)
    _C.cast_from_f32(d16, a)
    torch.cuda.synchronize()
    assert torch.equal(LU.raw_bits(d16), LU.raw_bits(a0.to(dtype))) and _outside_intact(draw, down, dtype)
    craw, cown, c = rows(torch.float32, 4)
    _C.add_f32(c, a, b)
    torch.cuda.synchronize()
    assert torch.equal(LU.raw_bits(c), LU.raw_bits(a0 + b0)) and _outside_intact(craw, cown, torch.float32)
    assert torch.equal(a, a0) and torch.equal(b, b0)
    _C.add_f32(a, a, b)                                       # dst aliases a
    _C.add_f32(b, a0.clone().copy_(a0), b)                    # (fresh a) dst aliases b
    torch.cuda.synchronize()
    assert torch.equal(LU.raw_bits(a), LU.raw_bits(a0 + b0)) and torch.equal(LU.raw_bits(b), LU.raw_bits(a0 + b0))
    assert _outside_intact(araw, aown, torch.float32) and _outside_intact(braw, bown, torch.float32)
    _note("cast / add", (), 1, 1)


def test_helper_kernels_second_grid_stride_pass(dev):
    """One launch of each HBM-bound helper above 2048 x 256 chunks (ew_grid's cap, usp_elementwise.hip): the grid-stride loop
    takes a second pass.  Every element checked."""
    from yunchang_amd import _C
    cap = 2048 * 256
    g = torch.Generator(device=dev).manual_seed(5)
    # copy: 16-byte chunks; sum: chunks of the destination
    n0, n1, row = 3, 1500, 1024                               # 3 * 1500 * 128 chunks = 576000
    assert n0 * n1 * row * 2 // 16 > cap
    src = torch.randn(2, n0, n1, row, device=dev, generator=g).to(torch.bfloat16)
    dst = torch.full((n0, n1, row + 8), float("nan"), dtype=torch.bfloat16, device=dev)
    _C.copy_rows(dst, src, row * 2, [n0, n1], [n1 * (row + 8) * 2, (row + 8) * 2], [n1 * row * 2, row * 2])
    assert torch.equal(dst[..., :row], src[0]) and bool(torch.isnan(dst[..., row:]).all())
    dst.fill_(float("nan"))
    _C.sum_rows(dst, src, row * 2, 2, n0 * n1 * row * 2, [n0, n1], [n1 * (row + 8) * 2, (row + 8) * 2], [n1 * row * 2, row * 2])
    assert torch.equal(dst[..., :row], (src[0].float() + src[1].float()).to(torch.bfloat16)) and bool(torch.isnan(dst[..., row:]).all())
    # cast: 8 elements per chunk; add: 4
    n = 8 * (cap + 3000)
    a, b = (torch.randn(1, 1, 1, n, device=dev, generator=g) for _ in range(2))
    d16 = torch.empty(1, 1, 1, n, dtype=torch.float16, device=dev)
    _C.cast_from_f32(d16, a)
    assert torch.equal(d16, a.to(torch.float16))
    c = torch.empty_like(a)
    _C.add_f32(c, a, b)
    assert torch.equal(c, a + b)
    # delta and merge: D / 8 lanes per row
    B, S, H, D = 2, 4300, 16, 32
    assert B * S * H * (D // 8) > cap
    do, o = (torch.randn(B, S, H, D, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
    delta = torch.full((B, H, S), float("nan"), device=dev)
    _C.bwd_delta(do, o, delta)
    want = (do.double() * o.double()).sum(-1).permute(0, 2, 1)
    assert_close(delta, want, 1e-4 * D ** 0.5, 1e-5, "delta, second grid-stride pass")
    acc = torch.randn(B, S, H, D, device=dev, generator=g)
    lse, bl = (torch.randn(B, H, S, device=dev, generator=g) for _ in range(2))
    ro, l4 = O.update_out_and_lse(acc.double().cpu().numpy(), lse.double().cpu().numpy().swapaxes(1, 2)[..., None],
                                  o.double().cpu().numpy(), bl.double().cpu().numpy())
    _C.lse_merge(acc, lse, o, bl, False)
    assert_close(acc.cpu().numpy(), ro, 1e-5, 1e-5, "merge acc, second grid-stride pass")
    assert_close(lse.cpu().numpy(), l4[..., 0].swapaxes(1, 2), 1e-5, 1e-5, "merge lse, second grid-stride pass")
    _note("helpers, 2nd grid-stride pass", (), 1, 1)


# ---- what the library refuses ----------------------------------------------------------------------------------------------------
def _padded(role, pad=1):
    return LU.Layout("row_pad", role, pad=pad)               # stride_h = D + 8 * pad: stride_s = H * (D + 8 pad), not a multiple of 128


def _fwd_tensors(dev, c, seed, layouts):
    q, k, v, _ = LU.make_inputs(c, seed)
    ar = LU.Arena(dev)
    tq, tk, tv = (LU.place(LU._tt(x, c.dt, dev), layouts[n], ar, n) for x, n in ((q, "q"), (k, "k"), (v, "v")))
    out = LU.blank((c.B, c.Sq, c.Hq, c.D), getattr(torch, c.dt), layouts["out"], ar, "out")
    lse = LU.blank((c.B, c.Hq, c.Sq), torch.float32, layouts["lse"], ar, "lse")
    return ar, tq, tk, tv, out, lse


def test_row64_stride_conditions_forward(dev):
    """USP_FORCE_ROW64 (include/usp_hip.h): the 64-row forward needs K's stride_s % 128 == 0 (its K pieces XOR their swizzle into
    the per-lane byte offset) and NOT V's (the V pieces' offsets are sums: usp_flash_fwd64.hip, v_voff / v_step)."""
    from yunchang_amd import _C
    c = LU.Case(2, 300, 333, 3, 1, 128, True, "bfloat16")
    names = ("q", "k", "v", "out", "lse")
    plain = LU.contiguous_layouts(names)
    ar, tq, tk, tv, out, lse = _fwd_tensors(dev, c, 1, dict(plain, k=_padded("in16")))
    assert tk.stride(1) % 128 != 0 and tk.stride(1) % 8 == 0
    with pytest.raises(RuntimeError, match="unsupported"):
        _C.flash_fwd(tq, tk, tv, c.scale, True, lse, out=out, family="row64", k_splits=0)
    torch.cuda.synchronize()
    assert _C.last_launch_kinds() == () and bool(LU.is_sentinel(out).all()) and bool(LU.is_sentinel(lse).all()) and ar.untouched()
    # unforced, the same call runs on the other family, bit-identical to a contiguous wave32 run
    _C.flash_fwd(tq, tk, tv, c.scale, True, lse, out=out, k_splits=0)
    kinds = _C.last_launch_kinds()
    assert kinds == ("fwd_wave4",), kinds
    ar2, q2, k2, v2, out2, lse2 = _fwd_tensors(dev, c, 1, plain)
    _C.flash_fwd(q2, k2, v2, c.scale, True, lse2, out=out2, family="wave32", k_splits=0)
    LU.assert_same_bits(out2, out, "unforced run with a padded K against the contiguous wave32 run: out")
    LU.assert_same_bits(lse2, lse, "unforced run with a padded K against the contiguous wave32 run: lse")
    # V alone with stride_s % 128 != 0: served by the 64-row kernel, bit-identical to its contiguous run
    base = {}
    for tag, lay in (("contig", plain), ("v padded", dict(plain, v=_padded("in16"))), ("v padded, cut", dict(plain, v=_padded("in16", 3)))):
        ar, tq, tk, tv, out, lse = _fwd_tensors(dev, c, 1, lay)
        ks = 3 if tag.endswith("cut") else 0
        assert tag == "contig" or (tv.stride(1) % 128 != 0 and tk.stride(1) % 128 == 0)
        _C.flash_fwd(tq, tk, tv, c.scale, True, lse, out=out, family="row64", k_splits=ks)
        torch.cuda.synchronize()
        assert _C.last_launch_kinds() == (("fwd_row64", "fwd_split_merge") if ks else ("fwd_row64",))
        assert ar.untouched() and ar.unchanged()
        if tag == "contig":
            base = dict(out=LU._host(out), lse=LU._host(lse))
            ro, rl = LU.ref_forward(c, *LU.make_inputs(c, 1)[:3])
            assert_close(LU._f64(out), ro, *TOL[c.dt]["out"], "row64 forward, contiguous")
        elif not ks:
            LU.assert_same_bits(base["out"], LU._host(out), f"row64 forward, {tag}: out")
            LU.assert_same_bits(base["lse"], LU._host(lse), f"row64 forward, {tag}: lse")
        else:
            ro, rl = LU.ref_forward(c, *LU.make_inputs(c, 1)[:3])
            assert_close(LU._f64(out), ro, *TOL[c.dt]["out"], f"row64 forward, {tag}")
    _note("refusals", [("fwd_row64", "fwd_split_merge", "fwd_wave4")], 1, 1)


@pytest.mark.parametrize("which", ["k", "v", "q", "dout"])
def test_row64_stride_conditions_backward(dev, which):
    """The 64-row dQ kernel needs stride_s % 128 == 0 on K and V, the 64-row dK/dV kernel on q and dout: forced, the call is
    refused and nothing is written; unforced, that launch runs on the 8-wave kernel and equals a contiguous wave32 run."""
    from yunchang_amd import _C
    only = "dq" if which in ("k", "v") else "dkdv"
    c = LU.Case(2, 200, 260, 2, 1, 128, True, "bfloat16", family="row64", only=only, forms=("h16", "f32", "h16"), dkdv_heads=2)
    lay = dict(LU.contiguous_layouts(LU.BWD_TENSORS), **{which: _padded("in16")})
    with pytest.raises(RuntimeError, match="unsupported"):
        LU.run_bwd(HipOps(), c, 3, dev, lay)
    assert _C.last_launch_kinds() == ()

    class Refused(HipOps):
        """Forced call: refused, every output still the sentinel; then the same tensors unforced."""
        def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, *a, **kw):
            with pytest.raises(RuntimeError, match="unsupported"):
                HipOps.bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, *a, **kw)
            torch.cuda.synchronize()
            for t in (dq, dk, dv, kw["dq16"], kw["dk16"], kw["dv16"]):
                assert t is None or bool(LU.is_sentinel(t).all()), "a refused call wrote an output"
            HipOps.bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, *a, **dict(kw, family=None))

    got = LU.run_bwd(Refused(), c, 3, dev, lay)
    assert set(got["kinds"]) == ({"dq_wave8"} if only == "dq" else {"dkdv_wave8"}), got["kinds"]
    c32 = LU.Case(2, 200, 260, 2, 1, 128, True, "bfloat16", family="wave32", only=only, forms=c.forms, dkdv_heads=2)
    base = LU.run_bwd(HipOps(), c32, 3, dev, LU.contiguous_layouts(LU.BWD_TENSORS))
    for n in base["wanted"]:
        LU.assert_same_bits(base[n], got[n], f"unforced backward with a padded {which} against the contiguous wave32 run: {n}")
    _note("refusals", [got["kinds"]], 1, 1)


def test_wave8_dkdv_32bit_offset_bound(dev):
    """The 8-wave dK/dV kernel addresses the Q / dO tiles of a head by a 32-bit byte offset: Sq * stride_s * 2 one 16-byte step
    below 2^31 is served and correct, at 2^31 the call is refused (include/usp_hip.h).  A sparse 2 GiB buffer: only the rows
    of the view and a guard band on either side of each are filled and checked."""
    from yunchang_amd import _C
    D, H, Sk, dt = 64, 1, 90, "bfloat16"
    G = 64                                                   # guard elements on either side of a row
    buf = torch.empty(2 ** 30 + 4096, dtype=torch.int16, device=dev)
    res = {}
    for tag, Sq, q_ss in (("contig", 511, D), ("below", 511, 8 * 262657), ("at", 512, 2 ** 21)):
        c = LU.Case(1, Sq, Sk, H, H, D, False, dt, family="wave32", only="dkdv", forms=("f32", "f32", "h16"))
        assert tag == "contig" or Sq * q_ss * 2 == 2 ** 31 - (16 if tag == "below" else 0)
        q, k, v, do = LU.make_inputs(c, 9)
        ro, rl = LU.ref_forward(c, q, k, v)
        o16 = LU.round_to(ro.astype(np.float32), dt)
        band = buf.as_strided((Sq, G + D + G), (q_ss, 1), 1024 - G)
        if tag != "contig":
            band.fill_(LU.SENTINEL[torch.bfloat16])
        tq = buf.view(torch.bfloat16).as_strided((1, Sq, H, D), (0, q_ss, D, 1), 1024) if tag != "contig" else None
        ar = LU.Arena(dev)
        if tq is None:
            tq = LU.place(LU._tt(q, dt, dev), LU.contiguous("in16"), ar, "q")
        else:
            tq.copy_(LU._tt(q, dt, dev))
        tdo, tk, tv, to = (LU.place(LU._tt(x, dt, dev), LU.contiguous("in16"), ar, n) for x, n in ((do, "dout"), (k, "k"), (v, "v"), (o16, "o")))
        lse = torch.from_numpy(np.ascontiguousarray(rl, dtype=np.float32)).to(dev)
        delta = torch.empty_like(lse)
        _C.bwd_delta(tdo, to, delta)
        dk = LU.blank(k.shape, torch.float32, LU.contiguous("f32"), ar, "dk")
        dv16 = LU.blank(k.shape, torch.bfloat16, LU.contiguous("out16"), ar, "dv16")
        call = lambda: _C.flash_bwd(tdo, tq, tk, tv, lse, delta, None, dk, None, c.scale, False, dv16=dv16, family="wave32",
                                    only="dkdv", splits=(0, 0))
        if tag == "at":
            with pytest.raises(RuntimeError, match="unsupported"):
                call()
            torch.cuda.synchronize()
            assert _C.last_launch_kinds() == () and bool(LU.is_sentinel(dk).all()) and bool(LU.is_sentinel(dv16).all())
            continue
        call()
        torch.cuda.synchronize()
        assert _C.last_launch_kinds() == ("dkdv_wave8",)
        assert ar.untouched() and ar.unchanged()
        if tag == "below":
            assert torch.equal(LU.raw_bits(tq), LU.raw_bits(LU._tt(q, dt, dev)[None][0])), "q was modified"
            guards = torch.cat([band[:, :G], band[:, G + D:]], 1)
            assert bool((guards == LU.SENTINEL[torch.bfloat16]).all()), "written beside a row of q"
        res[tag] = (LU._host(dk), LU._host(dv16))
        if tag == "contig":
            _, rdk, rdv = O.block_bwd(do, q, k, v, o16, rl, c.scale, False)
            assert_close(LU._f64(dk), rdk, *TOL[dt]["grad"], "dk")
            assert_close(LU._f64(dv16), rdv, *TOL[dt]["grad"], "dv")
    LU.assert_same_bits(res["contig"][0], res["below"][0], "Sq * stride_s * 2 = 2^31 - 16: dk")
    LU.assert_same_bits(res["contig"][1], res["below"][1], "Sq * stride_s * 2 = 2^31 - 16: dv")
    _note("refusals", [("dkdv_wave8",)], 1, 1)


# ---- report ------------------------------------------------------------------------------------------------------------------
def test_zz_every_cell_compared_what_it_drew_and_every_kernel_kind_ran_strided(dev, capsys):
    ran = set()
    with capsys.disabled():
        print("\nlayout sweeps: cell | drawn | bit-compared | launch kinds of the strided runs")
        for cell, r in REPORT.items():
            print(f"  {cell:32s} {r['drawn']:4d} {r['compared']:4d}  {' '.join(sorted(r['kinds']))}")
            ran |= r["kinds"]
    for cell, r in REPORT.items():
        assert r["drawn"] == r["compared"], f"{cell}: {r['drawn']} cases drawn, {r['compared']} compared"
    if all(REPORT.get(cell, {}).get("drawn") == N_OF.get(cell, N_CELL) for cell in CELLS):     # (not under a -k selection)
        assert ran >= set(ALL_KINDS), f"never launched strided: {set(ALL_KINDS) - ran}"
