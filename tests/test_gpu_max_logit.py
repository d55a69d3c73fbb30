"""return_max_logits on the GPU: flash_fwd_maxl_kernel (usp_flash_fwd_maxlogit) and usp_row_max_reduce against tests/max_logit_ref.py
(fp64, on the device; the tolerance is derived there) -- per row and per head, on white noise and on needle inputs, at the
smallest shapes that reach every loop of both workgroup shapes (pipelined interior tiles, the still unmasked tile that opens the
generic tail, causal / ragged / windowed tails, a shifted launch, rows that see nothing); merging launches over key halves and the
zigzag step pair with a `rows c:` slice; k_splits given and ignored; every tensor a strided view into a poisoned buffer; a
multi-pass launch against one workgroup per item; hip_attn_func's and the layer's autograd with a padded head dim under
sync-debug "error"; the rings and layers on one-device virtual grids; the 64-row family's refusal.

out and lse of a launch with the switch are compared BIT FOR BIT with the same launch without it (family="wave32": the same tile
loops).  Whether the row maxima of different tilings (4 / 8 waves, whole / key halves) are bit-equal is recorded ("MAXLBITS"),
not asserted: each score is one MFMA chain over D, so they should be.  Every comparison prints its error as a fraction of the
bound ("MAXLERR ...") before it asserts."""
import numpy as np
import pytest
import torch

import max_logit_ref as R
import needle_inputs as NI

pytestmark = pytest.mark.gpu

DTS = ("bfloat16", "float16")


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


# (id, B, Hq, Hkv, Sq, Sk, causal, window, shift, the kernel kind the dispatch picks)
# 4 waves: fewer than 256 items of 256 rows, or causal with Sq <= 1024; 8 waves: 256 items and more (usp_flash_fwd.hip: launch_fwd)
BLOCK_CASES = [
    ("c320", 2, 4, 2, 320, 320, True, None, None, "fwd_wave4"),           # 5 tiles: pipelined, then the diagonal ones
    ("c769", 2, 4, 2, 769, 769, True, None, None, "fwd_wave4"),           # ragged rows and keys, more than one block
    ("f129x513", 2, 4, 2, 129, 513, False, None, None, "fwd_wave4"),      # 8 full tiles pipelined + a ragged one; a 1-row wave
    ("f64", 2, 4, 2, 64, 64, False, None, None, "fwd_wave4"),             # one tile: no main loop at all
    ("f1x65", 2, 4, 2, 1, 65, False, None, None, "fwd_wave4"),
    ("w64_s512", 2, 4, 2, 512, 512, True, (64, 0), None, "fwd_wave4"),    # the window kernel's rotated walk
    ("shift", 2, 4, 2, 256, 384, True, None, -100, "fwd_wave4"),          # a shifted diagonal: rows 0 .. see 29 keys and more
    ("empty_rows", 2, 4, 2, 333, 200, True, None, None, "fwd_wave4"),     # rows 0 .. 132 see nothing
    ("empty_head", 1, 4, 2, 64, 64, True, None, -64, "fwd_wave4"),        # nothing visible at all: every head -inf
    ("w8_f129x513", 16, 16, 8, 129, 513, False, None, None, "fwd_wave8"),
    ("w8_f320", 8, 16, 8, 320, 320, False, None, None, "fwd_wave8"),
    ("w8_c1280", 4, 16, 8, 1280, 1280, True, None, None, "fwd_wave8"),    # 5 items a head; 20 tiles at the bottom
    ("w8_w64_s1280", 4, 16, 8, 1280, 1280, True, (64, 0), None, "fwd_wave8"),
]


def _white(dev, B, Sq, Sk, Hq, Hkv, D, dt, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, s, h, D, generator=g) for s, h in ((Sq, Hq), (Sk, Hkv), (Sk, Hkv)))
    return [t.to(getattr(torch, dt)).to(dev) for t in (q, k, v)]


def _needle(dev, B, Sq, Sk, Hq, Hkv, D, dt, seed):
    nd = NI.make(Sq, Sk, Hq, Hkv, D, dt, min(24, D - 2), seed=seed, B=B)
    return [torch.from_numpy(x).to(getattr(torch, dt)).to(dev) for x in (nd.q, nd.k, nd.v)]


def _fwd(q, k, v, scale, causal, row_max=None, lse=None, out=None, **kw):
    """One launch on the two-waves-per-SIMD family; NaN-prefilled results unless given."""
    from yunchang_amd import _C
    B, Sq, Hq, _ = q.shape
    out = torch.full_like(q, float("nan")) if out is None else out
    lse = torch.full((B, Hq, Sq), float("nan"), dtype=torch.float32, device=q.device) if lse is None else lse
    kw.setdefault("k_splits", 0)            # (the launch without row_max uncut too: the same tile loops, the same bits)
    _C.flash_fwd(q, k, v, scale, causal, lse, out=out, family="wave32", row_max=row_max, **kw)
    return out, lse, _C.last_launch_kinds()


def _nan_rows(B, Hq, Sq, dev):
    return torch.full((B, Hq, Sq), float("nan"), dtype=torch.float32, device=dev)


# white noise everywhere; needle inputs on the 4-wave cases and, at D = 128, on the deep 8-wave one
BLOCK_PARAMS = [pytest.param(c, D, dt, inputs, id=f"{c[0]}-D{D}-{dt}-{inputs}")
                for c in BLOCK_CASES for D in (32, 64, 128) for dt in DTS for inputs in ("white", "needle")
                if inputs == "white" or not c[0].startswith("w8_") or (c[0] == "w8_c1280" and D == 128)]


@pytest.mark.parametrize("case,D,dt,inputs", BLOCK_PARAMS)
def test_block(dev, case, D, dt, inputs):
    from yunchang_amd import _C
    name, B, Hq, Hkv, Sq, Sk, causal, window, shift, kind = case
    q, k, v = (_white if inputs == "white" else _needle)(dev, B, Sq, Sk, Hq, Hkv, D, dt, seed=Sq + D)
    scale = D ** -0.5
    kw = dict(window=window, shift=shift)
    rm = _nan_rows(B, Hq, Sq, dev)
    out, lse, kinds = _fwd(q, k, v, scale, causal, rm, **kw)
    assert kinds == (kind,), kinds
    out0, lse0, kinds0 = _fwd(q, k, v, scale, causal, None, **kw)
    assert kinds0[0] == kind
    assert torch.equal(out.view(torch.int16), out0.view(torch.int16)) and torch.equal(lse.view(torch.int32), lse0.view(torch.int32)), \
        "out / lse differ from the launch without row_max"
    ref = R.row_max_ref(q, k, scale, causal, window, shift or 0)
    pairs = R.abs_pairs(q, k)
    R.check(rm, ref, scale, D, pairs, f"rows {name} D{D} {dt} {inputs}")
    ml = _C.row_max_reduce(rm)
    assert torch.equal(ml, rm.amax(dim=(0, 2))), "usp_row_max_reduce is an exact maximum"
    R.check(ml, ref.amax(dim=(0, 2)), scale, D, pairs.amax(0), f"heads {name} D{D} {dt} {inputs}")
    if name in ("empty_rows",):
        assert bool(torch.isinf(rm[:, :, :133]).all()) and bool(torch.isfinite(rm[:, :, 133:]).all())
    if name == "empty_head":
        assert bool((ml == float("-inf")).all())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("D", [64, 128])
def test_row_max_is_tiling_independent(dev, D, dt):
    """The same problem on 4 and on 8 waves (interleave changes nothing of the kernel; the shape decides): B8 Hq16 S320 full runs 8
    waves, its first batch alone 4.  Recorded, and -- each score being one MFMA chain over D -- expected bit-equal."""
    q, k, v = _white(dev, 8, 320, 320, 16, 8, D, dt, seed=5)
    scale = D ** -0.5
    rm8, rm4 = _nan_rows(8, 16, 320, dev), _nan_rows(1, 16, 320, dev)
    assert _fwd(q, k, v, scale, False, rm8)[2] == ("fwd_wave8",)
    assert _fwd(q[:1], k[:1], v[:1], scale, False, rm4)[2] == ("fwd_wave4",)
    same = torch.equal(rm8[:1].view(torch.int32), rm4.view(torch.int32))
    print(f"MAXLBITS wave8 vs wave4 D{D} {dt}: {'bit-equal' if same else 'DIFFERENT'}")
    R.check(rm4, R.row_max_ref(q[:1], k[:1], scale), scale, D, R.abs_pairs(q[:1], k[:1]), "wave4 rows")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("D", [32, 64, 128])
def test_merging_launches_over_key_halves(dev, D, dt):
    """Keys [0, 320) then [320, 577) with merge_in: the second launch takes the maximum with what the first left.  Non-causal;
    and causal with the diagonal in the second half (shift keeps the global diagonal on the first)."""
    from yunchang_amd import _C
    B, Hq, Hkv, Sq, Sk, h = 2, 4, 2, 300, 577, 320
    q, k, v = _white(dev, B, Sq, Sk, Hq, Hkv, D, dt, seed=11)
    scale = D ** -0.5
    pairs = R.abs_pairs(q, k)
    for causal in (False, True):
        rm = _nan_rows(B, Hq, Sq, dev)
        lse = _nan_rows(B, Hq, Sq, dev)
        acc = torch.full(q.shape, float("nan"), dtype=torch.float32, device=dev)
        out = torch.full_like(q, float("nan"))
        # global row i sees global key j <= i + (Sk - Sq): the first half with the diagonal shifted by -(Sk - h)
        _C.flash_fwd(q, k[:, :h], v[:, :h], scale, causal, lse, out, acc, False, 0, 0, family="wave32", row_max=rm,
                     shift=(Sk - Sq) - (h - Sq) if causal else None)
        first = rm.clone()
        _C.flash_fwd(q, k[:, h:], v[:, h:], scale, causal, lse, out, acc, True, 0, Sq, family="wave32", row_max=rm)
        assert bool((rm >= first).all()), "a merging launch never lowers the maximum"
        ref = R.row_max_ref(q, k, scale, causal)
        R.check(rm, ref, scale, D, pairs, f"halves causal={causal} D{D} {dt}")
        whole = _nan_rows(B, Hq, Sq, dev)
        _fwd(q, k, v, scale, causal, whole)
        same = torch.equal(whole.view(torch.int32), rm.view(torch.int32))
        print(f"MAXLBITS halves vs whole causal={causal} D{D} {dt}: {'bit-equal' if same else 'DIFFERENT'}")


@pytest.mark.parametrize("dt", DTS)
def test_zigzag_step_pair_with_a_row_slice(dev, dt):
    """Ring rank 0 of 2 in the zigzag layout: step 0 causal over the 2c local rows, step 1 full on rows c: alone against the other
    rank's keys -- lse, out, acc and row_max all sliced alike.  Rows :c keep their value bit for bit."""
    from yunchang_amd import _C
    D, B, Hq, Hkv, c = 128, 1, 4, 2, 192
    q, k, v = _white(dev, B, 4 * c, 4 * c, Hq, Hkv, D, dt, seed=3)                     # the whole sequence: chunks 0 1 2 3
    scale = D ** -0.5
    loc = lambda t, a, b: torch.cat([t[:, a * c:(a + 1) * c], t[:, b * c:(b + 1) * c]], dim=1).contiguous()
    q0, k0, v0, k1, v1 = loc(q, 0, 3), loc(k, 0, 3), loc(v, 0, 3), loc(k, 1, 2), loc(v, 1, 2)
    rm, lse = _nan_rows(B, Hq, 2 * c, dev), _nan_rows(B, Hq, 2 * c, dev)
    out = torch.full_like(q0, float("nan"))
    acc = torch.full(q0.shape, float("nan"), dtype=torch.float32, device=dev)
    _C.flash_fwd(q0, k0, v0, scale, True, lse, out, acc, False, 0, c, family="wave32", row_max=rm)
    front = rm[:, :, :c].clone()
    _C.flash_fwd(q0[:, c:], k1, v1, scale, False, lse[:, :, c:], out[:, c:], acc[:, c:], True, 0, c, family="wave32",
                 row_max=rm[:, :, c:])
    assert torch.equal(front.view(torch.int32), rm[:, :, :c].view(torch.int32))
    ref = R.row_max_ref(q, k, scale, True)                                              # global rows: chunk 0 and chunk 3
    ref = torch.cat([ref[:, :, :c], ref[:, :, 3 * c:]], dim=2)
    R.check(rm, ref, scale, D, R.abs_pairs(q, k), f"zigzag pair {dt}")


@pytest.mark.parametrize("window", [None, (64, 0)])
def test_k_splits_given_and_ignored(dev, window):
    """k_splits = 4 with the switch: served uncut (no split-merge launch), the same bits as without cuts."""
    q, k, v = _white(dev, 1, 512, 2048, 4, 2, 128, "bfloat16", seed=9)
    scale = 128 ** -0.5
    a, b = _nan_rows(1, 4, 512, dev), _nan_rows(1, 4, 512, dev)
    o1, l1, kinds = _fwd(q, k, v, scale, True, a, k_splits=4, window=window)
    assert kinds == ("fwd_wave4",), kinds
    o2, l2, _ = _fwd(q, k, v, scale, True, b, k_splits=0, window=window)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(o1.view(torch.int16), o2.view(torch.int16))
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    R.check(a, R.row_max_ref(q, k, scale, True, window), scale, 128, R.abs_pairs(q, k), f"k_splits ignored window={window}")


def _strided(dev, shape, pad, dtype, fill, seed):
    """A view of `shape` with every stride but the last inflated by `pad`, inside a poisoned buffer with guard words around it:
    (view, the buffer, a bool mask of the elements the view owns)."""
    outer = [s + p for s, p in zip(shape[:-1], pad)] + [shape[-1] + 8]
    guard = 4096
    n = int(np.prod(outer))
    buf = torch.full((guard + n + guard,), fill, dtype=dtype, device=dev)
    body = buf[guard:guard + n].view(outer)
    view = body[tuple(slice(0, s) for s in shape)]
    own = torch.zeros(buf.shape, dtype=torch.bool, device=dev)
    own[guard:guard + n].view(outer)[tuple(slice(0, s) for s in shape)] = True
    return view, buf, own


@pytest.mark.parametrize("D,dt", [(64, "bfloat16"), (128, "float16")])
def test_strided_views_in_a_poisoned_buffer(dev, D, dt):
    """q, k, v, out, lse and row_max each a strided view of its own poisoned buffer: results as ever, and every word the views do
    not own keeps its poison."""
    B, Hq, Hkv, Sq, Sk = 2, 4, 2, 333, 400
    tdt = getattr(torch, dt)
    src = _white(dev, B, Sq, Sk, Hq, Hkv, D, dt, seed=21)
    ops, guards = [], []
    for t, pad in zip(src, ((1, 3, 2), (1, 5, 1), (2, 1, 3))):
        view, buf, own = _strided(dev, t.shape, pad, tdt, 777.0, 0)
        view.copy_(t)
        ops.append(view)
        guards.append((buf, own, buf.clone()))
    out, obuf, oown = _strided(dev, src[0].shape, (1, 2, 1), tdt, float("nan"), 0)
    lse, lbuf, lown = _strided(dev, (B, Hq, Sq), (1, 2), torch.float32, float("nan"), 0)
    rm, rbuf, rown = _strided(dev, (B, Hq, Sq), (2, 3), torch.float32, float("nan"), 0)
    scale = D ** -0.5
    _fwd(*ops, scale, True, rm, lse=lse, out=out)
    for buf, own, before in guards:
        assert torch.equal(buf.view(torch.int16), before.view(torch.int16)), "an operand was written"
    for buf, own, what in ((obuf, oown, "out"), (lbuf, lown, "lse"), (rbuf, rown, "row_max")):
        assert bool(torch.isnan(buf[~own]).all()), f"{what}: a guard word was written"
        assert not bool(torch.isnan(buf[own]).any()), f"{what}: an owned element was not written"
    R.check(rm, R.row_max_ref(*src[:2], scale, True), scale, D, R.abs_pairs(*src[:2]), f"strided D{D} {dt}")
    o0, l0, _ = _fwd(*src, scale, True, None)
    assert torch.equal(out.contiguous().view(torch.int16), o0.view(torch.int16)) and torch.equal(lse.contiguous().view(torch.int32), l0.view(torch.int32))


def test_multi_pass_launch_matches_one_workgroup_per_item(dev):
    """More items than resident workgroups (4 waves: two workgroups per CU; 8 waves: one), so every workgroup walks several items
    and m_true must start afresh with each: persistent against interleave=True (one workgroup per item), bit for bit."""
    from yunchang_amd import _C
    from yunchang_amd.comm.link import device_cus
    cus = device_cus()
    D, scale = 128, 128 ** -0.5
    for name, B, Hq, Hkv, S, causal, kind, slots in (("wave8", 2, 32, 8, 2048, True, "fwd_wave8", cus),
                                                     ("wave4", 8, 32, 8, 512, True, "fwd_wave4", 2 * cus)):
        items = B * Hq * ((S + (255 if kind == "fwd_wave8" else 127)) // (256 if kind == "fwd_wave8" else 128))
        assert items > slots, (items, slots)
        q, k, v = _white(dev, B, S, S, Hq, Hkv, D, "bfloat16", seed=2)
        a, b = _nan_rows(B, Hq, S, dev), _nan_rows(B, Hq, S, dev)
        o1, l1, kinds = _fwd(q, k, v, scale, causal, a)
        assert kinds == (kind,), kinds
        o2, l2, _ = _fwd(q, k, v, scale, causal, b, interleave=True)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
        assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)) and torch.equal(l1.view(torch.int32), l2.view(torch.int32))
        # the reference per batch: the dense fp64 score matrix of one batch at a time
        for bi in range(0, B, max(1, B // 2)):
            sl = slice(bi, bi + 1)
            R.check(a[sl], R.row_max_ref(q[sl], k[sl], scale, causal), scale, D, R.abs_pairs(q[sl], k[sl]), f"multi-pass {name} b{bi}")


def test_row64_family_declines_and_writes_nothing(dev):
    from yunchang_amd import _C
    q, k, v = _white(dev, 1, 256, 256, 4, 2, 128, "bfloat16", seed=1)
    out = torch.full_like(q, float("nan"))
    lse, rm = _nan_rows(1, 4, 256, dev), _nan_rows(1, 4, 256, dev)
    with pytest.raises(RuntimeError):
        _C.flash_fwd(q, k, v, 128 ** -0.5, True, lse, out=out, family="row64", row_max=rm)
    torch.cuda.synchronize()
    assert _C.last_launch_kinds() == ()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(lse).all()) and bool(torch.isnan(rm).all())
    # unforced, D = 128 at a size the 64-row family would take runs on the two-waves-per-SIMD kernels
    q, k, v = _white(dev, 2, 2048, 2048, 16, 8, 128, "bfloat16", seed=1)
    lse, rm = _nan_rows(2, 16, 2048, dev), _nan_rows(2, 16, 2048, dev)
    out = torch.empty_like(q)
    _C.flash_fwd(q, k, v, 128 ** -0.5, True, lse, out=out)
    assert _C.last_launch_kinds() == ("fwd_row64",)
    _C.flash_fwd(q, k, v, 128 ** -0.5, True, lse, out=out, row_max=rm)
    assert _C.last_launch_kinds() == ("fwd_wave8",)


@pytest.mark.parametrize("causal,window", [(True, (-1, -1)), (True, (100, 0)), (False, (-1, -1))])
def test_hip_attn_func_autograd(dev, causal, window):
    """hip_attn_func with a padded head dim (96 -> 128): out and the gradients are those of the call without the keyword, bit for
    bit; max_logits has no gradient and matches the reference on the UNPADDED operands (the padding changes no score); forward and
    backward run without a host read (sync-debug "error")."""
    from yunchang_amd import _C
    from yunchang_amd.kernels.attention import hip_attn_func
    B, S, Hq, Hkv, D = 2, 384, 4, 2, 96
    q, k, v = _white(dev, B, S, S, Hq, Hkv, D, "bfloat16", seed=4)
    do = torch.randn(B, S, Hq, D, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)
    family = _C.set_kernel_family("wave32")                  # the call without the keyword on the same tile loops
    try:
        grads = []
        for on in (False, True):
            a, b, c = (t.clone().requires_grad_(True) for t in (q, k, v))
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                res = hip_attn_func(a, b, c, causal=causal, window_size=window, return_max_logits=on)
                out, ml = res if on else (res, None)
                out.backward(do)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            grads.append((out.detach(), a.grad, b.grad, c.grad, ml))
    finally:
        _C.set_kernel_family(family)
    for x, y in zip(grads[0][:4], grads[1][:4]):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    ml = grads[1][4]
    assert ml.shape == (Hq,) and ml.dtype == torch.float32 and not ml.requires_grad
    win = None if window == (-1, -1) else window
    R.check(ml, R.max_logits_ref(q, k, D ** -0.5, causal, win), D ** -0.5, 128, R.abs_pairs(q, k).amax(0), f"hip_attn_func {causal} {window}")
    out, lse, none, ml2 = hip_attn_func(q, k, v, causal=causal, window_size=window, return_attn_probs=True, return_max_logits=True)
    assert none is None and lse.shape == (B, Hq, S) and torch.equal(ml2, ml)


# ---- the layer on a single-rank group, the rings and layers on one-device virtual grids --------------------------------------------
@pytest.fixture(scope="module")
def nccl_single():
    import os
    import torch.distributed as dist
    import yunchang_amd  # noqa: F401
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29747")
    own = not dist.is_initialized()
    if own:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    yield dist
    if own:
        dist.destroy_process_group()


@pytest.mark.parametrize("impl", ["basic", "zigzag", "strip"])
def test_layer_autograd_on_a_single_rank_group(dev, nccl_single, impl):
    """LongContextAttention on a 1 x 1 grid with a padded head dim (96): (out, max_logits); out and the gradients are those of the
    call without the keyword, bit for bit; forward and backward under sync-debug "error"."""
    import yunchang_amd as Y
    from yunchang_amd import _C
    Y.set_seq_parallel_pg(1, 1, 0, 1)
    B, S, Hq, Hkv, D = 2, 384, 4, 2, 96
    q, k, v = _white(dev, B, S, S, Hq, Hkv, D, "bfloat16", seed=6)
    do = torch.randn(B, S, Hq, D, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(dev)
    attn = Y.LongContextAttention(ring_impl_type=impl, attn_type=Y.AttnType.HIP)
    family = _C.set_kernel_family("wave32")
    try:
        runs = []
        for on in (False, True):
            a, b, c = (t.clone().requires_grad_(True) for t in (q, k, v))
            attn(a.detach(), b.detach(), c.detach(), causal=True, return_max_logits=on)      # (warm: groups and caches asked once)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                res = attn(a, b, c, causal=True, return_max_logits=on)
                out, ml = res if on else (res, None)
                out.backward(do)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            runs.append((out.detach(), a.grad, b.grad, c.grad, ml))
    finally:
        _C.set_kernel_family(family)
    for x, y in zip(runs[0][:4], runs[1][:4]):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    ml = runs[1][4]
    assert ml.shape == (Hq,) and ml.dtype == torch.float32 and not ml.requires_grad
    R.check(ml, R.max_logits_ref(q, k, D ** -0.5, True), D ** -0.5, 128, R.abs_pairs(q, k).amax(0), f"layer {impl}")


def _rows_of(impl, rank, ud, rd, S):
    """Global rows of rank = ring * ud + u (comm/extract_local.py)."""
    i, u = rank // ud, rank % ud
    if impl == "basic":
        n = S // (ud * rd)
        return torch.arange(rank * n, (rank + 1) * n)
    if impl == "strip":
        mine = torch.arange(i, S, rd)
    else:
        c = S // (2 * rd)
        mine = torch.cat([torch.arange(i * c, (i + 1) * c), torch.arange((2 * rd - 1 - i) * c, (2 * rd - i) * c)])
    n = mine.numel() // ud
    return mine[u * n:(u + 1) * n]


@pytest.mark.parametrize("impl", ["basic", "zigzag", "strip"])
@pytest.mark.parametrize("ud,rd", [(1, 2), (1, 4), (2, 1), (2, 2)])
def test_virtual_grids(dev, nccl_single, monkeypatch, ud, rd, impl):
    """Every rank of a ud x rd grid on one device: the head exchange, the ring's forward with max_logits, the share spread over
    the layer's heads (-inf where the rank holds no head).  The MAX over the ranks against the single-device call and the
    reference; every rank's out against the single-device out."""
    import yunchang_amd.comm.all_to_all as A
    import yunchang_amd.ring.ring_flash_attn as RB
    import yunchang_amd.ring.stripe_flash_attn as RS
    import yunchang_amd.ring.zigzag_ring_flash_attn as RZ
    from golden_util import TOL, assert_close
    from virtual_grid import VirtualGridPairwise, patch_dist, run_grid
    from yunchang_amd.kernels.attention import hip_attn_func
    fwd = {"basic": RB.ring_flash_attn_forward, "zigzag": RZ.zigzag_ring_flash_attn_forward, "strip": RS.stripe_flash_attn_forward}[impl]
    grid = VirtualGridPairwise(ud, rd, nccl_single)
    patch_dist(monkeypatch, grid)
    ws, D, rows, dt, Hq, Hkv = ud * rd, 64, 128, "bfloat16", 4, 2
    S = rows * ws
    q, k, v = _white(dev, 1, S, S, Hq, Hkv, D, dt, seed=8)
    idx = [_rows_of(impl, r, ud, rd, S).to(dev) for r in range(ws)]
    loc = [[t[:, idx[r]].contiguous() for t in (q, k, v)] for r in range(ws)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(ws)]
    scale = D ** -0.5
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        upg, rpg = grid.groups_of(r)
        lq, lk, lv = loc[r]
        with torch.cuda.stream(streams[r]):
            hq = A.heads_to_seq(lq, upg, contiguous=True)
            hk, hv = (A.kv_heads_to_seq(t, upg, contiguous=True) for t in (lk, lv))
            out, lse, ml = fwd(rpg, hq, hk, hv, scale, causal=True, max_logits=True)
            return [A.seq_to_heads(out, upg), A.layer_max_logits(ml, Hq, ud, r % ud)]
    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    one, ml_one = hip_attn_func(q, k, v, causal=True, return_max_logits=True)
    ref = R.max_logits_ref(q, k, scale, True)
    pairs = R.abs_pairs(q, k).amax(0)
    shares = torch.stack([res[r][1] for r in range(ws)])
    for r in range(ws):
        mine = torch.zeros(Hq, dtype=torch.bool, device=dev)
        mine[A.local_heads(Hq, ud, r % ud)] = True
        assert bool((shares[r][~mine] == float("-inf")).all()) and bool(torch.isfinite(shares[r][mine]).all()), (r, shares[r])
        assert_close(res[r][0].float(), one[:, idx[r]].double(), *TOL[dt]["out"], f"{impl} {ud}x{rd} rank {r} out")
    got = shares.amax(0)
    R.check(got, ref, scale, D, pairs, f"grid {impl} {ud}x{rd}")
    print(f"MAXLBITS grid {impl} {ud}x{rd} vs single device: {'bit-equal' if torch.equal(got, ml_one) else 'DIFFERENT'}")
    R.check(ml_one, ref, scale, D, pairs, "single device")
