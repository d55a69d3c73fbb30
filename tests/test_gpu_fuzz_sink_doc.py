"""Randomised GPU sweeps of the attention sinks and the document mask, the two options tests/test_gpu_fuzz.py::test_fuzz_features
does not rotate through, on the ragged shapes of its dense sweep (Sq, Sk in [1, 700), every head dim, both dtypes, Hkv in {1, 2, 3}
x group in {1, 2, 4}, B up to 3) against tests/doc_ref.py / tests/sink_ref.py (fp64, on the device).  Seeds are fixed: failures
reproduce.  Every call is launched twice, the second time with interleave=True and every tensor an independently drawn strided
view inside one sentinel arena (tests/layout_util.py), and must give the same bits.

test_fuzz_doc     the (row_lo, key_hi) arrays of tests/stair_inputs.py -- even seeds: cut out of document lists by the library's
                  planner, odd seeds: staircases, which is what the ABI admits beyond documents -- on needle inputs on which one
                  step of an array is an O(1) error (tests/test_fuzz_inputs_cpu.py shows that with the reference alone).  The
                  arrays reach the kernels as ring/doc_blocks.py: DocCall.upload hands them over: views at a 4-byte-aligned
                  offset into one int32 buffer, here between poison.
test_fuzz_sinks   the shapes, shifts, windows, K splits, cuts and dkdv_heads of the shifted sweep with per-head sinks, the ring's
                  step pair and usp_sink_bwd.

Every tolerance is the feature's own GPU test's (tests/test_gpu_doc_mask.py, tests/test_gpu_sink.py): `doc_tol`, `sink_tol`; each
comparison prints its largest error as a fraction of its tolerance ("[fuzz-doc-err]", "[fuzz-sinks-err]") before it asserts."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import doc_ref
import needle_inputs
import sink_ref
import stair_inputs as SI
from golden_util import TOL, assert_close, grad_tol, long_sum_atol, round_to
from test_gpu_fuzz import _dense_case, _err_line, _shifted_case

pytestmark = pytest.mark.gpu

_N_DOC = int(os.environ.get("USP_FUZZ_DOC", "24"))            # half lists, half staircases; larger sweeps: USP_FUZZ_DOC=400
_N_SINKS = int(os.environ.get("USP_FUZZ_SINKS", "18"))        # larger sweeps: USP_FUZZ_SINKS=300
_WAVE_FWD = {"fwd_wave8", "fwd_wave4"}
_WAVE_BWD = {"dkdv_wave8", "dq_wave8", "reduce_heads"}
_I32 = np.iinfo(np.int32)


@pytest.fixture(scope="module")
def dev():
    from yunchang_amd import _C
    _C.load()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _dev16(x, dt, device):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(getattr(torch, dt)).to(device)


def _bits_equal(a, b):
    import layout_util as LU
    return torch.equal(LU.raw_bits(a), LU.raw_bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# the cases, their inputs and their tolerances: host code, shared with tests/test_fuzz_inputs_cpu.py
# ---------------------------------------------------------------------------------------------------------------------
def doc_case(seed):
    """One case of test_fuzz_doc.  The shape is _dense_case's (its window, K split and cuts are not used); every further draw
    comes after it: the arrays; `dkdv_heads` from the divisors of the group; in a third of the cases each: only="dq" / "dkdv"
    launches, a K split and backward cuts (which the document launches must ignore), and -- full blocks only -- the ring
    contract (keys of a first plain launch, final_begin, final_end); 16-bit or fp32 gradient outputs."""
    rs = np.random.RandomState(21000 + seed)
    B, Sq, Sk, Hq, Hkv, D, causal, dt = _dense_case(rs)[:8]
    launch = SI.draw_doc_launch(rs, B, Sq, Sk) if seed % 2 == 0 else SI.draw_stair_launch(rs, B, Sq, Sk, causal)
    Sq, Sk = launch.Sq, launch.Sk
    G = Hq // Hkv
    heads = int(rs.choice([g for g in range(1, G + 1) if G % g == 0]))
    only = bool(rs.rand() < 1.0 / 3)
    ks, splits = int(rs.choice([2, 3, 5])), ((2, 2), (3, 4))[int(rs.randint(2))]
    cut = (ks, splits) if rs.rand() < 1.0 / 3 else None
    n0, fb = int(rs.randint(1, 200)), int(rs.randint(0, Sq + 1))
    fe = int(rs.randint(fb, Sq + 1))
    ring = (n0, fb, fe) if (rs.rand() < 1.0 / 3 and not launch.causal) else None
    out16 = bool(rs.rand() < 0.5)
    what = (f"doc seed {seed} {launch.kind} B{B} Sq{Sq} Sk{Sk} Hq{Hq} Hkv{Hkv} D{D} causal={launch.causal} {dt} "
            f"{'one array' if launch.shared else 'arrays per entry'} empty={launch.empty} plateaus="
            f"{[len(SI.plateaus(r)) for r in np.asarray(launch.row_lo).reshape(-1, Sq)]} dkdv_heads={heads} only={only} cut={cut} "
            f"ring={ring} out16={out16}")
    return SimpleNamespace(rs=rs, seed=seed, launch=launch, B=B, Sq=Sq, Sk=Sk, Hq=Hq, Hkv=Hkv, D=D, G=G, dt=dt, causal=launch.causal,
                           heads=heads, only=only, cut=cut, ring=ring, out16=out16, what=what)


def doc_inputs(c):
    """Needle inputs (tests/needle_inputs.py, C = 8) with the edges of every array of the launch."""
    return needle_inputs.make(c.Sq, c.Sk, c.Hq, c.Hkv, c.D, c.dt, C=8, seed=c.seed, B=c.B, edges=SI.launch_edges(c.launch))


def doc_tol(name, dt, G, Sq, Sk, want):
    """(atol, rtol) of tests/test_gpu_doc_mask.py: TOL[dt]["out"], the lse at 2e-3 + 1e-4 |lse|, gradients at grad_tol -- with
    golden_util.long_sum_atol as _run_dense applies it (dQ sums Sk keys, dK / dV sum Sq * G rows)."""
    if name == "out":
        return TOL[dt]["out"]
    if name == "lse":
        return 2e-3, 1e-4
    atol, rtol = grad_tol(dt, G)
    return long_sum_atol(atol, Sk if name == "dq" else Sq * G, want), rtol


def sink_tol(name, dt, G, Sq, Sk, want):
    """(atol, rtol) of tests/test_gpu_sink.py: out and lse at TOL[dt]["out"], gradients at grad_tol, with long_sum_atol."""
    return TOL[dt]["out"] if name in ("out", "lse") else doc_tol(name, dt, G, Sq, Sk, want)


def sink_case(seed):
    """One case of test_fuzz_sinks: _shifted_case (the forced 64-row family declines sinks: "wave32" instead, as _feature_case
    does), then the sinks, the ring's step pair in a third of the cases (the keys cut at a drawn position) and q, k ~ N(0, 1)."""
    rs = np.random.RandomState(17000 + seed)
    (B, Sq, Sk, Hq, Hkv, D, causal, dt, win, ks, cuts), shift, heads, family = _shifted_case(rs)
    family = "wave32" if family == "row64" else family
    sinks = SI.draw_sinks(rs, Hq)
    pair, at = bool(rs.rand() < 1.0 / 3), int(rs.randint(1, max(2, Sk)))
    q, k = (round_to(rs.standard_normal(s).astype(np.float32), dt) for s in [(B, Sq, Hq, D), (B, Sk, Hkv, D)])
    what = (f"sinks seed {seed} {sinks.tolist()} B{B} Sq{Sq} Sk{Sk} Hq{Hq} Hkv{Hkv} D{D} causal={causal} {dt} window={win} k_splits={ks} "
            f"cuts={cuts} shift={shift} dkdv_heads={heads} family={family} pair={at if pair and Sk >= 2 else None}")
    return SimpleNamespace(rs=rs, seed=seed, B=B, Sq=Sq, Sk=Sk, Hq=Hq, Hkv=Hkv, D=D, G=Hq // Hkv, causal=causal, dt=dt, win=win, ks=ks,
                           cuts=cuts, shift=shift, heads=heads, family=family, sinks=sinks, pair=at if pair and Sk >= 2 else None,
                           q=q, k=k, what=what)


_REDRAWS = {}                                                  # seed -> draws of v / dout the case needed beyond the first


def sink_inputs(c, device):
    """(q, k, v, dout, sinks) on `device`, the fp64 reference there and sum |terms| of ds per head.  v, dout ~ N(1, 1)
    (tests/test_gpu_sink.py): delta has one sign and the terms of ds_h do not cancel -- asserted on the reference
    (_terms_not_cancelling); a case that fails it draws v / dout again with the next seed offset, and none is dropped."""
    from test_gpu_sink import _terms_not_cancelling
    q, k = _dev16(c.q, c.dt, device), _dev16(c.k, c.dt, device)
    s = torch.from_numpy(c.sinks).to(device)
    for attempt in range(4):
        rs = np.random.RandomState(17000 + c.seed + 100003 * (attempt + 1))
        v, do = (_dev16(round_to((rs.standard_normal(sh) + 1.0).astype(np.float32), c.dt), c.dt, device)
                 for sh in [(c.B, c.Sk, c.Hkv, c.D), (c.B, c.Sq, c.Hq, c.D)])
        ref = sink_ref.ref_bwd(do, q, k, v, c.D ** -0.5, s, c.causal, c.win, c.shift, out_dtype=q.dtype)
        try:
            tot = _terms_not_cancelling(s, ref, do, c.dt)
        except AssertionError:
            continue
        _REDRAWS[c.seed] = attempt
        return (q, k, v, do, s), ref, tot
    raise AssertionError(c.what + ": the terms of ds cancel in four draws of v / dout")


def redraw_cap_holds():
    """At most one case in six needed another draw of v / dout."""
    return 6 * sum(1 for n in _REDRAWS.values() if n) <= max(len(_REDRAWS), 6)


# ---------------------------------------------------------------------------------------------------------------------
# the document mask
# ---------------------------------------------------------------------------------------------------------------------
def _doc_arena(rs, launch, device):
    """row_lo and key_hi as contiguous views into ONE int32 buffer, each at an offset that is a multiple of 4 bytes and not of
    16, the rest INT32_MIN / INT32_MAX -> (row_lo view, key_hi view, buffer, its host copy)."""
    rl, kh = np.asarray(launch.row_lo), np.asarray(launch.key_hi)
    o1 = 4 * int(rs.randint(1, 8)) + int(rs.randint(1, 4))
    o2 = o1 + rl.size + int(rs.randint(1, 32))
    o2 += 1 if o2 % 4 == 0 else 0
    host = np.where(np.arange(o2 + kh.size + int(rs.randint(4, 32))) % 2 == 0, _I32.min, _I32.max).astype(np.int32)
    host[o1:o1 + rl.size], host[o2:o2 + kh.size] = rl.reshape(-1), kh.reshape(-1)
    buf = torch.from_numpy(host).to(device)
    views = [buf[o:o + a.size].view(a.shape) for o, a in ((o1, rl), (o2, kh))]
    for t in views:
        assert t.is_contiguous() and t.data_ptr() % 4 == 0 and t.data_ptr() % 16 != 0
    return views[0], views[1], buf, torch.from_numpy(host.copy())


@pytest.mark.parametrize("seed", range(_N_DOC))
def test_fuzz_doc(dev, seed):
    """usp_flash_fwd_doc / usp_flash_bwd_doc on drawn arrays: bit-identity of two launches in independent layouts; out, lse, dq,
    dk, dv against the fp64 reference under doc_ref.block_mask; rows that see nothing exactly 0 / -inf; the launch kinds; `only`
    launches with the unused array None; a K split and cuts ignored bit for bit; the ring contract (merge_in after a plain
    launch over other keys, a drawn final range); the buffer that holds the arrays untouched."""
    from yunchang_amd import _C
    import layout_util as LU
    c = doc_case(seed)
    rs, what, la = c.rs, c.what, c.launch
    B, Sq, Sk, Hq, Hkv, D, G, dt, causal = c.B, c.Sq, c.Sk, c.Hq, c.Hkv, c.D, c.G, c.dt, c.causal
    nd = doc_inputs(c)
    tq, tk, tv, tdo = (_dev16(x, dt, dev) for x in (nd.q, nd.k, nd.v, nd.do))
    scale, dtype = D ** -0.5, tq.dtype
    mask = doc_ref.block_mask(la.row_lo, Sq, Sk, causal, B)
    ref = doc_ref.ref_bwd(tdo, tq, tk, tv, scale, mask, out_dtype=dtype)
    rl, kh, buf, buf_host = _doc_arena(rs, la, dev)
    doc = (rl, kh)
    lay = lambda name: LU.draw_layout(rs, LU.ROLE[name], B)      # (drawn last: after the shape, the arrays and the options)
    arena = LU.Arena(dev)
    # ---- forward: contiguous, then interleave + an independent layout per tensor
    out = torch.full((B, Sq, Hq, D), float("nan"), dtype=dtype, device=dev)
    lse = torch.full((B, Hq, Sq), float("nan"), dtype=torch.float32, device=dev)
    _C.flash_fwd(tq, tk, tv, scale, causal, lse, out=out, doc=doc)
    kinds = _C.last_launch_kinds()
    assert kinds and set(kinds) <= _WAVE_FWD, (what, kinds)
    sq, sk, sv, sdo = (LU.place(t, lay(n), arena, n) for t, n in ((tq, "q"), (tk, "k"), (tv, "v"), (tdo, "dout")))
    out2 = LU.blank((B, Sq, Hq, D), dtype, lay("out"), arena, "out")
    lse2 = LU.blank((B, Hq, Sq), torch.float32, lay("lse"), arena, "lse")
    _C.flash_fwd(sq, sk, sv, scale, causal, lse2, out=out2, interleave=True, doc=doc)
    assert _bits_equal(out, out2) and _bits_equal(lse, lse2), f"{what}: the forward differs between two launches"
    if c.cut:                                                    # k_splits is IGNORED with the arrays (include/usp_hip.h)
        out3, lse3 = torch.full_like(out, float("nan")), torch.full_like(lse, float("nan"))
        _C.flash_fwd(tq, tk, tv, scale, causal, lse3, out=out3, doc=doc, k_splits=c.cut[0])
        kinds = _C.last_launch_kinds()
        assert kinds and set(kinds) <= _WAVE_FWD, (what, kinds)
        assert _bits_equal(out, out3) and _bits_equal(lse, lse3), f"{what}: k_splits={c.cut[0]} changes the forward"
    for got, want, name in ((out, ref[0], "out"), (lse, ref[1], "lse")):
        tol = doc_tol(name, dt, G, Sq, Sk, want)
        _err_line("fuzz-doc", what, name, got, want, *tol)
        assert_close(got, want, *tol, f"{what} {name}")
    empty = ~mask.any(-1).to(dev)                                # (B, Sq): rows that see nothing
    assert bool((out[empty] == 0).all()) and bool(torch.isneginf(lse.transpose(1, 2)[empty]).all()), \
        f"{what}: rows that see nothing must give out = 0, lse = -inf"
    # ---- backward: lse from the reference, delta from the 16-bit-rounded reference out
    lse_t = ref[1].to(torch.float32)
    delta = torch.empty((B, Hq, Sq), dtype=torch.float32, device=dev)
    _C.bwd_delta(tdo, ref[0].to(dtype), delta)
    gdt, names = (dtype, ("dq16", "dk16", "dv16")) if c.out16 else (torch.float32, ("dq", "dk", "dv"))

    def bwd(do_, q_, k_, v_, lse_, delta_, g, doc_, **kw):
        a32, a16 = ((None, None, None), g) if c.out16 else (g, (None, None, None))
        _C.flash_bwd(do_, q_, k_, v_, lse_, delta_, *a32, scale, causal, dq16=a16[0], dk16=a16[1], dv16=a16[2], doc=doc_,
                     dkdv_heads=c.heads, **kw)
        return _C.last_launch_kinds()
    fresh = lambda: [torch.full(t.shape, float("nan"), dtype=gdt, device=dev) for t in (tq, tk, tv)]
    g1 = fresh()
    kinds = bwd(tdo, tq, tk, tv, lse_t, delta, g1, doc)
    assert {"dkdv_wave8", "dq_wave8"} <= set(kinds) <= _WAVE_BWD, (what, kinds)
    assert "reduce_heads" not in kinds or c.heads < G, (what, kinds)
    slse, sdelta = LU.place(lse_t, lay("lse"), arena, "lse_in"), LU.place(delta, lay("delta"), arena, "delta")
    g2 = [LU.blank(tuple(t.shape), gdt, lay(n), arena, n) for t, n in zip((tq, tk, tv), names)]
    bwd(sdo, sq, sk, sv, slse, sdelta, g2, doc, interleave=True)
    for a_, b_, n_ in zip(g1, g2, ("dq", "dk", "dv")):
        assert _bits_equal(a_, b_), f"{what}: {n_} differs between two launches"
    bad = arena.violations()
    assert not bad, f"{what}: written outside the views: {bad}"
    assert arena.unchanged(), what + ": an input view was modified"
    if c.only:                                                   # each launch alone, the array it does not read None
        for only, doc_, live in (("dq", (rl, None), (0,)), ("dkdv", (None, kh), (1, 2))):
            g3 = fresh()
            kinds = bwd(tdo, tq, tk, tv, lse_t, delta, g3, doc_, only=only)
            assert kinds and set(kinds) <= _WAVE_BWD and ("dq_wave8" in kinds) == (only == "dq"), (what, only, kinds)
            for i, n_ in enumerate(("dq", "dk", "dv")):
                if i in live:
                    assert _bits_equal(g1[i], g3[i]), f"{what}: {n_} of only={only} differs from the full call"
                else:
                    assert bool(torch.isnan(g3[i]).all()), f"{what}: only={only} wrote {n_}"
    if c.cut:                                                    # dq_splits / dkdv_splits are IGNORED with the arrays
        g4 = fresh()
        kinds = bwd(tdo, tq, tk, tv, lse_t, delta, g4, doc, splits=c.cut[1])
        assert {"dkdv_wave8", "dq_wave8"} <= set(kinds) <= _WAVE_BWD, (what, kinds)
        for a_, b_, n_ in zip(g1, g4, ("dq", "dk", "dv")):
            assert _bits_equal(a_, b_), f"{what}: splits={c.cut[1]} changes {n_}"
    for g_, r_, n_ in zip(g1, ref[2:], ("dq", "dk", "dv")):
        tol = doc_tol(n_, dt, G, Sq, Sk, r_)
        _err_line("fuzz-doc", what, n_, g_, r_, *tol)
        assert_close(g_, r_, *tol, f"{what} {n_}")
    assert bool((g1[0][empty] == 0).all()), f"{what}: rows that see nothing must give dq = 0"
    if c.ring:
        _ring_contract(dev, c, rs, (tq, tk, tv), mask, doc, what)
    assert torch.equal(buf.cpu(), buf_host), what + ": the buffer that holds row_lo / key_hi was modified"


def _ring_contract(dev, c, rs, qkv, mask, doc, what):
    """A ring's later step (tests/test_gpu_doc_mask.py::test_full_block_with_left_bound[merge_in]): a first plain launch over
    other keys opens the rows' state in acc / lse, the document launch merges into it with a drawn final range.  Against the
    reference over the concatenated keys; rows whose bound is Sk leave the second launch with the first launch's state."""
    from yunchang_amd import _C
    q, k, v = qkv
    n0, fb, fe = c.ring
    B, Sq, Hq, D, dt, scale = c.B, c.Sq, c.Hq, c.D, c.dt, c.D ** -0.5
    k0, v0 = (_dev16(round_to(rs.standard_normal((B, n0, c.Hkv, D)).astype(np.float32), dt), dt, dev) for _ in range(2))
    acc = torch.full(q.shape, float("nan"), dtype=torch.float32, device=dev)
    lse = torch.full((B, Hq, Sq), float("nan"), dtype=torch.float32, device=dev)
    out = torch.full_like(q, float("nan"))
    _C.flash_fwd(q, k0, v0, scale, False, lse, out=out, acc=acc, final_begin=0, final_end=0, family="wave32")
    acc1, lse1 = acc.clone(), lse.clone()
    _C.flash_fwd(q, k, v, scale, False, lse, out=out, acc=acc, merge_in=True, final_begin=fb, final_end=fe, doc=doc)
    kinds = _C.last_launch_kinds()
    assert kinds and set(kinds) <= _WAVE_FWD, (what, kinds)
    m2 = torch.cat([torch.ones(B, Sq, n0, dtype=torch.bool), mask], dim=2)
    want = doc_ref.ref_fwd(q, torch.cat([k0, k], 1), torch.cat([v0, v], 1), scale, m2)
    final = torch.zeros(Sq, dtype=torch.bool, device=dev)
    final[fb:fe] = True
    for got, w, name in ((out[:, final], want[0][:, final], "ring out (final rows)"), (acc[:, ~final], want[0][:, ~final], "ring acc"),
                         (lse, want[1], "ring lse")):
        tol = doc_tol("lse" if name == "ring lse" else "out", dt, c.G, Sq, c.Sk, w)
        _err_line("fuzz-doc", what, name, got, w, *tol)
        assert_close(got, w, *tol, f"{what} {name}")
    blind = torch.from_numpy(np.asarray(c.launch.row_lo).reshape(-1, Sq) == c.Sk).to(dev).expand(B, Sq)      # bound = Sk
    assert _bits_equal(lse.transpose(1, 2)[blind], lse1.transpose(1, 2)[blind]), f"{what}: a row that sees nothing here changed its lse"
    assert _bits_equal(acc[blind & ~final], acc1[blind & ~final]), f"{what}: a row that sees nothing here changed its acc"
    assert _bits_equal(out[blind & final], acc1[blind & final].to(q.dtype)), f"{what}: a final row that sees nothing here is not its acc"


# ---------------------------------------------------------------------------------------------------------------------
# the sinks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(_N_SINKS))
def test_fuzz_sinks(dev, seed):
    """usp_flash_fwd_sink with the shifts, windows, K splits, cuts and dkdv_heads the case draws: bit-identity of two launches in
    independent layouts (of a gradient: where one kernel served both launches, see below); out, lse, dq, dk, dv against tests/sink_ref.py; rows without a key exactly lse = sinks[h], out = 0; a K
    split merges (fwd_split_merge) and counts the sink once; the ring's step pair against the one-shot reference; usp_sink_bwd
    on the kernel's own lse."""
    from yunchang_amd import _C
    import layout_util as LU
    from test_gpu_sink import _check_empty_rows
    c = sink_case(seed)
    rs, what = c.rs, c.what
    B, Sq, Sk, Hq, Hkv, D, G, dt, causal = c.B, c.Sq, c.Sk, c.Hq, c.Hkv, c.D, c.G, c.dt, c.causal
    (tq, tk, tv, tdo, s), ref, tot = sink_inputs(c, dev)
    print(f"[fuzz-sinks-redraw] {what}: {_REDRAWS[seed]} further draws of v / dout")
    assert redraw_cap_holds(), f"more than one case in six drew v / dout again: {_REDRAWS}"
    scale, dtype = D ** -0.5, tq.dtype
    wkw = dict(shift=c.shift, family=c.family, **({} if c.win is None else {"window": c.win}))
    lay = lambda name: LU.draw_layout(rs, LU.ROLE[name], B)      # (drawn last)
    arena = LU.Arena(dev)
    # ---- forward
    out = torch.full((B, Sq, Hq, D), float("nan"), dtype=dtype, device=dev)
    lse = torch.full((B, Hq, Sq), float("nan"), dtype=torch.float32, device=dev)
    _C.flash_fwd(tq, tk, tv, scale, causal, lse, out=out, k_splits=c.ks, sinks=s, **wkw)
    kinds = _C.last_launch_kinds()
    assert kinds and set(kinds) - {"fwd_split_merge"} <= _WAVE_FWD and ("fwd_split_merge" in kinds) == (c.ks > 1), (what, kinds)
    sq, sk, sv, sdo = (LU.place(t, lay(n), arena, n) for t, n in ((tq, "q"), (tk, "k"), (tv, "v"), (tdo, "dout")))
    out2 = LU.blank((B, Sq, Hq, D), dtype, lay("out"), arena, "out")
    lse2 = LU.blank((B, Hq, Sq), torch.float32, lay("lse"), arena, "lse")
    _C.flash_fwd(sq, sk, sv, scale, causal, lse2, out=out2, interleave=True, k_splits=c.ks, sinks=s, **wkw)
    assert _bits_equal(out, out2) and _bits_equal(lse, lse2), f"{what}: the forward differs between two launches"
    for got, want, name in ((out, ref[0], "out"), (lse, ref[1], "lse")):
        tol = sink_tol(name, dt, G, Sq, Sk, want)
        _err_line("fuzz-sinks", what, name, got, want, *tol)
        assert_close(got, want, *tol, f"{what} {name}")
    n_empty = _check_empty_rows(out, lse, s, Sq, Sk, causal, c.win, c.shift)
    # ---- backward: usp_flash_bwd fed the sink-including lse of the reference, delta from the 16-bit-rounded reference out
    lse_t = ref[1].to(torch.float32)
    delta = torch.empty((B, Hq, Sq), dtype=torch.float32, device=dev)
    _C.bwd_delta(tdo, ref[0].to(dtype), delta)
    g1 = [torch.full_like(t, float("nan")) for t in (tq, tk, tv)]
    _C.flash_bwd(tdo, tq, tk, tv, lse_t, delta, None, None, None, scale, causal, dq16=g1[0], dk16=g1[1], dv16=g1[2],
                 splits=c.cuts, dkdv_heads=c.heads, **wkw)
    kinds1 = _C.last_launch_kinds()
    slse, sdelta = LU.place(lse_t, lay("lse"), arena, "lse_in"), LU.place(delta, lay("delta"), arena, "delta")
    g2 = [LU.blank(tuple(t.shape), dtype, lay(n), arena, n) for t, n in ((tq, "dq16"), (tk, "dk16"), (tv, "dv16"))]
    _C.flash_bwd(sdo, sq, sk, sv, slse, sdelta, None, None, None, scale, causal, dq16=g2[0], dk16=g2[1], dv16=g2[2],
                 interleave=True, splits=c.cuts, dkdv_heads=c.heads, **wkw)
    kinds2 = _C.last_launch_kinds()
    # An unforced D = 128 backward runs the 64-row kernels where the rows of its streamed tensors lie a multiple of 256 bytes
    # apart (dkdv64_serves: q, dout; dq64_serves: k, v) and the two-waves-per-SIMD ones elsewhere: the drawn layouts of the second
    # launch may send one of its two kernels to the other family.  Bit-identity is that of ONE kernel; a gradient another
    # kernel served is held against the reference like the first launch's.
    served = lambda kinds, pre: {x for x in kinds if x.startswith(pre)}
    same = {"dq": served(kinds1, "dq_") == served(kinds2, "dq_"), "dk": served(kinds1, "dkdv_") == served(kinds2, "dkdv_")}
    same["dv"] = same["dk"]
    assert all(same.values()) or (c.family is None and D == 128), (what, kinds1, kinds2)
    for a_, b_, n_ in zip(g1, g2, ("dq", "dk", "dv")):
        assert not same[n_] or _bits_equal(a_, b_), f"{what}: {n_} differs between two launches"
    bad = arena.violations()
    assert not bad, f"{what}: written outside the views: {bad}"
    assert arena.unchanged(), what + ": an input view was modified"
    for g_, g2_, r_, n_ in zip(g1, g2, ref[2:5], ("dq", "dk", "dv")):
        tol = sink_tol(n_, dt, G, Sq, Sk, r_)
        _err_line("fuzz-sinks", what, n_, g_, r_, *tol)
        assert_close(g_, r_, *tol, f"{what} {n_}")
        if not same[n_]:
            _err_line("fuzz-sinks", what, f"{n_} (second launch: {sorted(kinds2)} after {sorted(kinds1)})", g2_, r_, *tol)
            assert_close(g2_, r_, *tol, f"{what} {n_} of the second launch")
    # ---- usp_sink_bwd on the kernel's OWN lse and the backward's delta
    terms = sink_ref.sink_terms(s, lse, delta)
    own, gate = -terms.sum(dim=(0, 2)), 2.0 ** -17 * terms.abs().sum(dim=(0, 2))
    ds = _C.sink_grad(s, lse, delta)
    err = (ds.double() - own).abs()
    print(f"[fuzz-sinks-err] {what} dsinks vs the formula on the same lse / delta: {float((err / gate).nan_to_num(0.0).max()):.3f} of tolerance")
    assert bool((err <= gate).all()), (what, err, gate)
    err, gate = (ds.double() - ref[5]).abs(), TOL[dt]["grad"][1] * tot
    print(f"[fuzz-sinks-err] {what} dsinks vs truth: {float((err / gate).nan_to_num(0.0).max()):.3f} of tolerance ({n_empty} empty rows)")
    assert bool((err <= gate).all()), (what, err, gate, ds, ref[5])
    # ---- the ring's step pair: the first keys WITH sinks to acc, the others merged in without; the mask of the one-shot call on
    #      both (row i sees key j by j - i alone: launch 1 ends Sk - at keys early, so its diagonal moves by that much)
    if c.pair is not None:
        at = c.pair
        acc = torch.full(tq.shape, float("nan"), dtype=torch.float32, device=dev)
        lse_p = torch.full_like(lse, float("nan"))
        out_p = torch.full_like(out, float("nan"))
        _C.flash_fwd(tq, tk[:, :at], tv[:, :at], scale, causal, lse_p, acc=acc, final_begin=0, final_end=0, k_splits=c.ks, sinks=s,
                     **dict(wkw, shift=c.shift + Sk - at))
        kinds = _C.last_launch_kinds()
        assert ("fwd_split_merge" in kinds) == (c.ks > 1), (what, kinds)
        _C.flash_fwd(tq, tk[:, at:], tv[:, at:], scale, causal, lse_p, out=out_p, acc=acc, merge_in=True, **wkw)
        for got, want, name in ((out_p, ref[0], "out"), (lse_p, ref[1], "lse")):
            tol = sink_tol(name, dt, G, Sq, Sk, want)
            _err_line("fuzz-sinks", what, "step pair " + name, got, want, *tol)
            assert_close(got, want, *tol, f"{what} step pair {name}")
