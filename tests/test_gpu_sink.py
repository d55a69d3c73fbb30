"""Attention sinks (sinks) on the GPU: flash_fwd_sink_kernel (usp_flash_fwd_sink) and usp_sink_bwd against tests/sink_ref.py (fp64,
on the device) -- block parity with empty rows, windows and a shifted launch, the K split (the sink counted once), the eight-wave
kernel and the family dispatch, a ring step pair composed at kernel level, independent layouts, the sink gradient alone,
hip_attn_func's autograd, the basic and zigzag rings on virtual ranks, and sinks=None through every entry point.

v and dout are drawn as N(1, 1): delta_i = dout_i . out_i then has one sign and the terms of ds_h do not cancel (asserted on the
reference: |ds_h| >= 0.5 sum |terms|), so a gate relative to sum |terms| is a gate relative to the gradient.  Per-head sinks
(-30, 0, +3, +12): no effect, off-by-one softmax, a strong sink, a sink above every score.  Every comparison prints its largest
error as a fraction of its gate ("SINKERR ...") before it asserts."""
import os

import numpy as np
import pytest
import torch

import sink_ref
from golden_util import TOL, assert_close, grad_tol

pytestmark = pytest.mark.gpu

B, HQ, HKV = 2, 4, 2
SINKS = (-30.0, 0.0, 3.0, 12.0)
SHAPES = [(200, 333), (333, 200), (77, 77), (512, 700)]      # (Sq, Sk); (333, 200) has rows without a key under causal


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _case(dev, Bc, Sq, Sk, Hq, Hkv, D, dt, seed=0):
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(Bc, s, h, D, generator=g) for s, h in ((Sq, Hq), (Sk, Hkv), (Sk, Hkv), (Sq, Hq)))
    return [t.to(getattr(torch, dt)).to(dev) for t in (q, k, v + 1.0, do + 1.0)]


def _sinks(dev, H=HQ):
    return torch.tensor(SINKS * (H // 4), dtype=torch.float32, device=dev)


_REF, _IN = {}, {}


def _inputs(dev, Sq, Sk, D, dt):
    key = (Sq, Sk, D, dt)
    if key not in _IN:
        _IN[key] = _case(dev, B, Sq, Sk, HQ, HKV, D, dt, seed=Sq + D)
    return _IN[key]


def _reference(key, do, q, k, v, scale, sinks, causal=False, window=None, shift=0):
    """(out, lse, dq, dk, dv, dsinks) fp64 on the device, computed once per case and shared (never modified)."""
    if key not in _REF:
        _REF[key] = sink_ref.ref_bwd(do, q, k, v, scale, sinks, causal, window, shift, out_dtype=q.dtype)
    return _REF[key]


def _close(got, want, atol, rtol, what):
    frac = float(((got.double() - want.double()).abs() / (atol + rtol * want.double().abs())).nan_to_num(nan=float("inf")).max())
    print(f"SINKERR {what} {frac:.3f}")
    assert_close(got, want, atol, rtol, what)


def _run_fwd(q, k, v, scale, causal, sinks, **kw):
    from yunchang_amd import _C
    out = torch.full_like(q, float("nan"))
    lse = torch.full((q.shape[0], q.shape[2], q.shape[1]), float("nan"), dtype=torch.float32, device=q.device)
    _C.flash_fwd(q, k, v, scale, causal, lse, out=out, sinks=sinks, **kw)
    return out, lse, _C.last_launch_kinds()


def _run_bwd(do, q, k, v, ref, scale, causal, **kw):
    """usp_flash_bwd, unchanged, fed the sink-including lse: that IS the backward."""
    from yunchang_amd import _C
    lse = ref[1].to(torch.float32)
    delta = torch.empty_like(lse)
    _C.bwd_delta(do, ref[0].to(q.dtype), delta)
    dq, dk, dv = (torch.full(t.shape, float("nan"), dtype=torch.float32, device=q.device) for t in (q, k, v))
    _C.flash_bwd(do, q, k, v, lse, delta, dq, dk, dv, scale, causal, **kw)
    return dq, dk, dv


def _check_fwd(out, lse, ref, dt, what):
    _close(out, ref[0], *TOL[dt]["out"], f"{what} out")
    _close(lse, ref[1], *TOL[dt]["out"], f"{what} lse")


def _check_bwd(grads, ref, dt, what):
    for g, r, name in zip(grads, ref[2:5], ("dq", "dk", "dv")):
        _close(g, r, *grad_tol(dt, HQ // HKV), f"{what} {name}")


def _check_empty_rows(out, lse, sinks, Sq, Sk, causal, window=None, shift=0):
    """A row without a visible key: lse == sinks[h] EXACTLY and out == 0."""
    empty = ~sink_ref.alibi_ref.visible(Sq, Sk, causal, window, shift, out.device).any(1)
    if bool(empty.any()):
        assert torch.equal(lse[:, :, empty], sinks[None, :, None].expand(lse.shape[0], -1, int(empty.sum())))
        assert not bool(out[:, empty].float().abs().any())
    return int(empty.sum())


def _terms_not_cancelling(sinks, ref, do, dt):
    delta = (do.double() * ref[0].to(getattr(torch, dt)).double()).sum(-1).transpose(1, 2)
    tot = sink_ref.sink_terms(sinks, ref[1], delta).abs().sum(dim=(0, 2))
    assert bool((ref[5].abs() >= 0.5 * tot).all()), (ref[5], tot)
    return tot


_WAVE = {"fwd_wave8", "fwd_wave4"}


# ---- 1. block parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sq,Sk", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_block_parity(dev, D, dt, causal, Sq, Sk):
    q, k, v, do = _inputs(dev, Sq, Sk, D, dt)
    scale, s = D ** -0.5, _sinks(dev)
    ref = _reference(("blk", D, dt, causal, Sq, Sk), do, q, k, v, scale, s, causal)
    _terms_not_cancelling(s, ref, do, dt)
    what = f"D{D} {dt} causal {causal} {Sq}x{Sk}"
    out, lse, kinds = _run_fwd(q, k, v, scale, causal, s)
    assert kinds and set(kinds) <= _WAVE, kinds
    _check_fwd(out, lse, ref, dt, what)
    assert (_check_empty_rows(out, lse, s, Sq, Sk, causal) > 0) == (causal and Sq > Sk)
    _check_bwd(_run_bwd(do, q, k, v, ref, scale, causal), ref, dt, what)


# ---- 2. windows (the rotated walk of the window instantiation) and a shifted launch -------------------------------------------
@pytest.mark.parametrize("window,shift,causal", [((17, 0), None, True), ((128, 0), None, True), ((128, 40), None, False),
                                                 ((40, 0), -60, True), ((40, 0), -150, True)], ids=lambda v: str(v))
@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
def test_window_and_shift(dev, dt, window, shift, causal):
    D, (Sq, Sk) = 64, ((200, 333) if shift is not None else (333, 459))
    q, k, v, do = _inputs(dev, Sq, Sk, D, dt)
    scale, s = D ** -0.5, _sinks(dev)
    ref = _reference(("win", dt, window, shift, causal), do, q, k, v, scale, s, causal, window, shift or 0)
    what = f"D{D} {dt} window {window} shift {shift}"
    kw = {} if shift is None else {"shift": shift}
    out, lse, kinds = _run_fwd(q, k, v, scale, causal, s, window=window, **kw)
    assert kinds and set(kinds) <= _WAVE, kinds
    _check_fwd(out, lse, ref, dt, what)
    assert (_check_empty_rows(out, lse, s, Sq, Sk, causal, window, shift or 0) > 0) == (shift == -150)
    _check_bwd(_run_bwd(do, q, k, v, ref, scale, causal, window=window, **kw), ref, dt, what)


# ---- 3. the K split: cut 0 alone carries the sink -----------------------------------------------------------------------------
@pytest.mark.parametrize("D,dt,window", [(128, "bfloat16", None), (64, "float16", None), (64, "bfloat16", (300, 0))], ids=lambda v: str(v))
def test_k_split_counts_the_sink_once(dev, D, dt, window):
    Sq, Sk, causal = 512, 700, True
    q, k, v, do = _inputs(dev, Sq, Sk, D, dt)
    scale, s = D ** -0.5, _sinks(dev)
    ref = _reference(("split", D, dt, window), do, q, k, v, scale, s, causal, window)
    o1, l1, kinds = _run_fwd(q, k, v, scale, causal, s, k_splits=0, window=window)
    assert "fwd_split_merge" not in kinds
    _check_fwd(o1, l1, ref, dt, f"unsplit D{D} {dt} {window}")
    for n in (2, 3):
        o, l, kinds = _run_fwd(q, k, v, scale, causal, s, k_splits=n, window=window)
        assert "fwd_split_merge" in kinds and set(kinds) - {"fwd_split_merge"} <= _WAVE, kinds
        _check_fwd(o, l, ref, dt, f"k_splits {n} D{D} {dt} {window}")
        _close(o, o1.double(), *TOL[dt]["out"], f"k_splits {n} vs unsplit out")
        _close(l, l1.double(), *TOL[dt]["out"], f"k_splits {n} vs unsplit lse")
    # ... and into the fp32 accumulator (final_end = 0), where the merge launch writes acc
    from yunchang_amd import _C
    acc = torch.full(q.shape, float("nan"), dtype=torch.float32, device=dev)
    lse = torch.full_like(l1, float("nan"))
    _C.flash_fwd(q, k, v, scale, causal, lse, acc=acc, final_end=0, k_splits=2, sinks=s, window=window)
    _close(acc, ref[0], *TOL[dt]["out"], "k_splits 2 to acc")
    _close(lse, ref[1], *TOL[dt]["out"], "k_splits 2 to acc lse")


def test_automatic_k_split(dev):
    """B1 Hq4 S4096 causal: fwd_k_splits cuts every item in four; the result is the unsplit one."""
    from yunchang_amd import _C
    D, dt, S = 64, "bfloat16", 4096
    assert _C.fwd_k_splits(1, S, HQ, True) == 4
    q, k, v, _ = _case(dev, 1, S, S, HQ, HKV, D, dt, seed=9)
    scale, s = D ** -0.5, _sinks(dev)
    o1, l1, kinds1 = _run_fwd(q, k, v, scale, True, s, k_splits=0)
    o, l, kinds = _run_fwd(q, k, v, scale, True, s)
    assert "fwd_split_merge" in kinds and "fwd_split_merge" not in kinds1, (kinds, kinds1)
    ro, rl = sink_ref.ref_fwd(q, k, v, scale, s, True)
    _check_fwd(o, l, (ro, rl), dt, "automatic split")
    _close(o, o1.double(), *TOL[dt]["out"], "automatic split vs unsplit out")
    _close(l, l1.double(), *TOL[dt]["out"], "automatic split vs unsplit lse")


# ---- 4. the eight-wave kernel and the family dispatch ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
def test_eight_wave_kernel_and_dispatch(dev, D):
    """B2 Hq16 S2048: 256 items of 256 rows.  D = 64: fwd_wave8.  D = 128: a plain launch takes the 64-row family here; with sinks
    it stays on the two-waves-per-SIMD family, unforced."""
    dt, S, H = "bfloat16", 2048, 16
    q, k, v, _ = _case(dev, 2, S, S, H, 4, D, dt, seed=D)
    scale, s = D ** -0.5, _sinks(dev, H)
    out, lse, kinds = _run_fwd(q, k, v, scale, True, s)
    assert kinds == ("fwd_wave8",), kinds
    _check_fwd(out, lse, sink_ref.ref_fwd(q, k, v, scale, s, True), dt, f"wave8 D{D}")
    if D == 128:
        _, _, plain = _run_fwd(q, k, v, scale, True, None)
        assert plain == ("fwd_row64",), plain


def test_row64_family_declines_and_writes_nothing(dev):
    from yunchang_amd import _C
    q, k, v, _ = _inputs(dev, 200, 333, 128, "bfloat16")
    out = torch.full_like(q, float("nan"))
    lse = torch.full((B, HQ, 200), float("nan"), dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match="unsupported"):
        _C.flash_fwd(q, k, v, 128 ** -0.5, True, lse, out=out, sinks=_sinks(dev), family="row64")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(lse).all()) and _C.last_launch_kinds() == ()
    with pytest.raises(RuntimeError, match="invalid"):       # merge_in: the sink belongs to the launch that opens the rows
        _C.flash_fwd(q, k, v, 128 ** -0.5, True, lse, out=out, acc=torch.zeros(q.shape, device=dev), merge_in=True, sinks=_sinks(dev))


# ---- 5. a ring's step pair at kernel level ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dt", [(64, "bfloat16"), (128, "float16")])
def test_ring_composition_at_kernel_level(dev, D, dt):
    """Launch 1: merge_in = 0, to acc, the first keys, WITH sinks.  Launch 2: merge_in = 1, the other keys, final, without.  The
    pair is the one-shot reference over all keys."""
    from yunchang_amd import _C
    Sq, Sk, cut = 200, 333, 160
    q, k, v, do = _inputs(dev, Sq, Sk, D, dt)
    scale, s = D ** -0.5, _sinks(dev)
    ref = _reference(("blk", D, dt, False, Sq, Sk), do, q, k, v, scale, s, False)
    out = torch.full_like(q, float("nan"))
    acc = torch.full(q.shape, float("nan"), dtype=torch.float32, device=dev)
    lse = torch.full((B, HQ, Sq), float("nan"), dtype=torch.float32, device=dev)
    _C.flash_fwd(q, k[:, :cut], v[:, :cut], scale, False, lse, acc=acc, merge_in=False, final_begin=0, final_end=0, sinks=s)
    _C.flash_fwd(q, k[:, cut:], v[:, cut:], scale, False, lse, out=out, acc=acc, merge_in=True)
    _check_fwd(out, lse, ref, dt, f"step pair D{D} {dt}")


# ---- 6. every tensor in a layout of its own -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [0, 1, 2])
def test_independent_layouts(dev, index):
    import layout_util as LU
    from yunchang_amd import _C
    D, dt, Sq, Sk = 64, "bfloat16", 200, 333
    q, k, v, _ = _inputs(dev, Sq, Sk, D, dt)
    scale, s = D ** -0.5, _sinks(dev)
    o0, l0, _ = _run_fwd(q, k, v, scale, True, s)

    class C:
        B = 2
    arena = LU.Arena(dev)
    lay = LU.draw_layouts(np.random.RandomState(17 + index), C, ("q", "k", "v", "out", "lse"), index)
    pq, pk, pv = (LU.place(t, lay[n], arena, n) for t, n in ((q, "q"), (k, "k"), (v, "v")))
    po = LU.blank(tuple(q.shape), q.dtype, lay["out"], arena, "out")
    pl = LU.blank((B, HQ, Sq), torch.float32, lay["lse"], arena, "lse")
    _C.flash_fwd(pq, pk, pv, scale, True, pl, out=po, sinks=s)
    torch.cuda.synchronize()
    LU.assert_same_bits(po, o0, f"out under {lay}")
    LU.assert_same_bits(pl, l0, f"lse under {lay}")
    assert arena.untouched(), arena.violations()
    assert arena.unchanged()


# ---- 7. usp_sink_bwd alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bc,H,S", [(2, 4, 1000), (1, 3, 77), (3, 8, 5000)], ids=lambda v: str(v))
def test_sink_grad_alone(dev, Bc, H, S):
    """Against the fp64 evaluation of the formula on the SAME fp32 lse / delta: |err| <= 2^-17 sum |terms| per head (a tree sum
    over <= 2^20 terms errs by <~ 20 x 2^-24 sum |terms|, a few ulp for the exponential on top, ~4 x margin)."""
    from yunchang_amd import _C
    g = torch.Generator().manual_seed(S)
    lse = (torch.randn(Bc, H, S, generator=g) * 2 + 3).to(dev)
    delta = (torch.randn(Bc, H, S, generator=g) + 1).to(dev)
    lse[0, 0, ::7] = float("-inf")                           # such a term counts as 0, whatever its delta
    s = torch.tensor([(-30.0, 0.0, 3.0, 12.0, 1.5, -2.0, 6.0, 0.5)[h] for h in range(H)], device=dev)
    terms = sink_ref.sink_terms(s, lse, delta)
    want, bound = -terms.sum(dim=(0, 2)), 2.0 ** -17 * terms.abs().sum(dim=(0, 2))
    got = _C.sink_grad(s, lse, delta)
    assert got.dtype == torch.float32 and tuple(got.shape) == (H,)
    err = (got.double() - want).abs()
    print(f"SINKERR sink_grad B{Bc} H{H} S{S} {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (err, bound)
    again = torch.full((H,), float("nan"), device=dev)
    assert _C.sink_grad(s, lse, delta, out=again) is again and torch.equal(again, got)      # bit-identical: no atomics
    _C.sink_grad(s, lse, delta, out=again, accum=True)                                      # accum = 1 adds
    assert bool(((again.double() - 2 * want).abs() <= 2 * bound + 2.0 ** -23 * want.abs()).all())
    # strided lse / delta (their own batch and head strides, unit seq stride)
    big_l = torch.full((Bc, H + 1, S + 8), float("nan"), device=dev)
    big_d = torch.full((Bc + 1, H, S + 4), float("nan"), device=dev)
    big_l[:, 1:, 4:4 + S] = lse
    big_d[1:, :, :S] = delta
    assert torch.equal(_C.sink_grad(s, big_l[:, 1:, 4:4 + S], big_d[1:, :, :S]), got)
    with pytest.raises(ValueError):
        _C.sink_grad(s, lse, delta, accum=True)


# ---- 8. hip_attn_func: autograd, a padded head dim ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dt,sdt", [(96, "bfloat16", torch.float32), (64, "float16", torch.float32), (64, "bfloat16", torch.bfloat16)],
                         ids=lambda v: str(v))
def test_hip_attn_func_autograd(dev, D, dt, sdt):
    from yunchang_amd.kernels.attention import hip_attn_func, kernel_head_dim
    Sq = Sk = 300
    q, k, v, do = _case(dev, B, Sq, Sk, HQ, HKV, D, dt, seed=D)
    s32 = _sinks(dev)
    ref = sink_ref.ref_bwd(do, q, k, v, D ** -0.5, s32, True, out_dtype=q.dtype)
    tot = _terms_not_cancelling(s32, ref, do, dt)
    lq, lk, lv = (t.clone().requires_grad_(True) for t in (q, k, v))
    ls = s32.to(sdt).requires_grad_(True)
    out, lse, _ = hip_attn_func(lq, lk, lv, causal=True, return_attn_probs=True, sinks=ls)
    out.backward(do)
    what = f"hip_attn_func D{D} {dt}"
    _check_fwd(out.detach(), lse, ref, dt, what)
    _check_bwd((lq.grad, lk.grad, lv.grad), ref, dt, what)
    assert ls.grad.dtype == sdt and ls.grad.shape == ls.shape
    # (a) the formula fed the kernel's OWN out and lse: the sink kernel's gate + the fp32 error of the kernel's delta (a sum of
    #     kernel_head_dim products: <= Dp x 2^-24 x sum_d |dout_d out_d| per row) [+ the rounding of a 16-bit gradient]
    prod = do.double() * out.detach().double()
    delta = prod.sum(-1).transpose(1, 2)
    e = torch.exp(s32.double()[None, :, None] - lse.double())
    own = -(e * delta).sum(dim=(0, 2))
    gate = 2.0 ** -17 * (e * delta).abs().sum(dim=(0, 2)) + \
        (e * (kernel_head_dim(D) * 2.0 ** -24 * prod.abs().sum(-1).transpose(1, 2))).sum(dim=(0, 2))
    if sdt != torch.float32:
        gate = gate + 2.0 ** -8 * own.abs()
    err = (ls.grad.double() - own.detach()).abs()
    print(f"SINKERR {what} dsinks vs own formula {float((err / gate).detach().max()):.3f}")
    assert bool((err <= gate).all()), (err, gate)
    # (b) the fp64 truth of the whole problem: rtol of the gradients x sum |terms|
    err = (ls.grad.double() - ref[5]).abs()
    gate = TOL[dt]["grad"][1] * tot
    print(f"SINKERR {what} dsinks vs truth {float((err / gate).max()):.3f}")
    assert bool((err <= gate).all()), (err, gate, ls.grad, ref[5])


# ---- 9. the rings on virtual ranks -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nccl_single():
    import torch.distributed as dist
    import yunchang_amd  # noqa: F401
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29743")
    own = not dist.is_initialized()
    if own:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    yield dist
    if own:
        dist.destroy_process_group()


def _rows_of(impl, rank, ud, rd, S):
    """Global rows of rank = ring * ud + u (comm/extract_local.py; the extract functions ask torch.distributed for the grid)."""
    i, u = rank // ud, rank % ud
    if impl == "basic":
        n = S // (ud * rd)
        return torch.arange(rank * n, (rank + 1) * n)
    c = S // (2 * rd)
    mine = torch.cat([torch.arange(i * c, (i + 1) * c), torch.arange((2 * rd - 1 - i) * c, (2 * rd - i) * c)])
    n = mine.numel() // ud
    return mine[u * n:(u + 1) * n]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("impl", ["basic", "zigzag"])
@pytest.mark.parametrize("ud,rd", [(1, 2), (2, 2), (1, 4)])
def test_grid_invariance_on_virtual_ranks(dev, nccl_single, monkeypatch, ud, rd, impl):
    """Every rank's out, dq, dk, dv against ONE single-device hip_attn_func call on the unsharded tensors; the ranks' shares of
    dsinks -- their rows, their heads -- sum to the single-device gradient."""
    import yunchang_amd.comm.all_to_all as A
    import yunchang_amd.ring.ring_flash_attn as R
    import yunchang_amd.ring.zigzag_ring_flash_attn as Z
    from virtual_grid import VirtualGridPairwise, patch_dist, run_grid
    from yunchang_amd.kernels import get_block_backend
    from yunchang_amd.kernels.attention import hip_attn_func
    assert get_block_backend().name == "hip"
    fwd, bwd = {"basic": (R.ring_flash_attn_forward, R.ring_flash_attn_backward),
                "zigzag": (Z.zigzag_ring_flash_attn_forward, Z.zigzag_ring_flash_attn_backward)}[impl]
    grid = VirtualGridPairwise(ud, rd, nccl_single)
    patch_dist(monkeypatch, grid)
    ws, D, rows, dt = ud * rd, 64, 128, "bfloat16"
    S = rows * ws
    q, k, v, do = _case(dev, 1, S, S, HQ, HKV, D, dt, seed=4)
    s = _sinks(dev)
    idx = [_rows_of(impl, r, ud, rd, S).to(dev) for r in range(ws)]
    loc = [[t[:, idx[r]].contiguous() for t in (q, k, v, do)] for r in range(ws)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(ws)]
    scale = D ** -0.5
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        upg, rpg = grid.groups_of(r)
        lq, lk, lv, ldo = loc[r]
        hs = A.local_heads(HQ, ud, r % ud)
        kw = dict(causal=True, sinks=A.local_sinks(s, HQ, ud, r % ud))
        with torch.cuda.stream(streams[r]):
            hq, hdo = (A.heads_to_seq(t, upg, contiguous=True) for t in (lq, ldo))
            hk, hv = (A.kv_heads_to_seq(t, upg, contiguous=True) for t in (lk, lv))
            out, lse = fwd(rpg, hq, hk, hv, scale, **kw)
            dq, dk, dv, ds = bwd(rpg, hdo, hq, hk, hv, out, lse, scale, **kw)
            share = torch.zeros(HQ, dtype=torch.float32, device=dev)
            share[hs] = ds
            return [A.seq_to_heads(out, upg), A.seq_to_heads(dq, upg), A.kv_seq_to_heads(dk, upg, HKV),
                    A.kv_seq_to_heads(dv, upg, HKV), share]
    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v, s)]
    one = hip_attn_func(*leaves[:3], causal=True, sinks=leaves[3])
    one.backward(do)
    single = (one.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad)
    for r in range(ws):
        for got, want, name in zip(res[r], single, ("out", "dq", "dk", "dv")):
            tol = TOL[dt]["out"] if name == "out" else grad_tol(dt, HQ // HKV)
            _close(got.float(), want[:, idx[r]].double(), *tol, f"{impl} {ud}x{rd} rank {r} {name}")
    ref = sink_ref.ref_bwd(do, q, k, v, scale, s, True, out_dtype=q.dtype)
    tot = _terms_not_cancelling(s, ref, do, dt)
    summed = torch.stack([res[r][4] for r in range(ws)]).double().sum(0)
    gate = TOL[dt]["grad"][1] * tot
    for name, want in (("single device", leaves[3].grad.double()), ("truth", ref[5])):
        err = (summed - want).abs()
        print(f"SINKERR {impl} {ud}x{rd} summed dsinks vs {name} {float((err / gate).max()):.3f}")
        assert bool((err <= gate).all()), (name, summed, want, gate)


# ---- 10. sinks = None is the plain path, bit for bit -------------------------------------------------------------------------------------
def test_plain_path_unchanged(dev, nccl_single):
    import yunchang_amd as Y
    from yunchang_amd import _C
    from yunchang_amd.kernels.attention import hip_attn_backward, hip_attn_forward, hip_attn_func
    q, k, v, do = _inputs(dev, 333, 459, 128, "bfloat16")
    scale = 128 ** -0.5
    a = _run_fwd(q, k, v, scale, True, None)
    out = torch.full_like(q, float("nan"))
    lse = torch.full_like(a[1], float("nan"))
    _C.flash_fwd(q, k, v, scale, True, lse, out=out)
    assert a[2] == _C.last_launch_kinds() and torch.equal(a[0], out) and torch.equal(a[1], lse)
    o1, l1 = hip_attn_forward(q, k, v, causal=True, sinks=None)
    o2, l2 = hip_attn_forward(q, k, v, causal=True)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    g1, g2 = ([torch.empty_like(t) for t in (q, k, v)] for _ in range(2))
    hip_attn_backward(do, q, k, v, o1, l1, *g1, bwd_causal=True, sinks=None)
    hip_attn_backward(do, q, k, v, o1, l1, *g2, bwd_causal=True)
    assert all(torch.equal(x, y) for x, y in zip(g1, g2))
    Y.set_seq_parallel_pg(1, 1, 0, 1)
    sq, sk, sv, sdo = _inputs(dev, 512, 512, 64, "bfloat16")
    layer = Y.LongContextAttention(ring_impl_type="zigzag", attn_type=Y.AttnType.HIP)
    calls = [lambda a, b, c, kw: hip_attn_func(a, b, c, causal=True, **kw),
             lambda a, b, c, kw: Y.ring_flash_attn_func(a, b, c, causal=True, **kw),
             lambda a, b, c, kw: Y.zigzag_ring_flash_attn_func(a, b, c, causal=True, **kw),
             lambda a, b, c, kw: Y.stripe_flash_attn_func(a, b, c, causal=True, **kw),
             lambda a, b, c, kw: layer(a, b, c, causal=True, **kw)]
    for call in calls:
        got = []
        for kw in ({"sinks": None}, {}):
            leaves = [t.clone().requires_grad_(True) for t in (sq, sk, sv)]
            o = call(*leaves, kw)
            kinds = _C.last_launch_kinds()
            o.backward(sdo)
            got.append((kinds, o.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad))
        assert got[0][0] == got[1][0], (got[0][0], got[1][0])
        assert all(torch.equal(x, y) for x, y in zip(got[0][1:], got[1][1:]))
