"""A sliding window over GLOBAL positions on the basic ring, GPU side: the block kernels with a shifted mask diagonal
(USP_ATTN_SHIFT) against tests/shift_ref.py, windowed launches whose query tiles have left-cut, interior and right-cut key tiles,
the ring forward / backward of USP_RING_WINDOW=global on virtual ranks (real kernels, real RCCL self send/recv) and on two
processes sharing the GPU.

Inputs are N(0,1): with at most 1280 keys per row a lost 64-key TILE is at least 5 % of a row's mass, far outside TOL
(SURVEY.md section 8(c)), so white noise is not blind to tiles at these sizes.  It IS blind to single keys: with windows of
327, 500 or 700 keys one key is 0.14 - 0.3 % of a row's mass, so an off-by-one in causal_off + shift or win_lo + shift passes
every N(0,1) test of this file.  Key-exactness of the shifted masks is pinned on needle inputs, in tests/test_gpu_needle.py
(`SHIFTED`, `RING_BLOCKS`) and tests/test_gpu_mutation.py, not here; the ring itself runs on needle inputs in
`test_global_window_on_virtual_ranks_with_needle_inputs` below.  The extreme window bounds and shifts at the end of the file
are O(1) effects (everything or nothing visible): white noise suffices there."""
import os

import pytest
import torch

import shift_ref
from dist_util import run_distributed
from golden_util import TOL, assert_close, grad_tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _case(dev, B, Sq, Sk, Hq, Hkv, D, dt, seed=0):
    g = torch.Generator().manual_seed(seed)
    dtype = getattr(torch, dt)
    return [torch.randn(B, s, h, D, generator=g).to(dtype).to(dev) for s, h in ((Sq, Hq), (Sk, Hkv), (Sk, Hkv), (Sq, Hq))]


_REF = {}


def _reference(key, q, k, v, do, scale, causal, window, shift, softcap=None):
    """(out, lse, dq, dk, dv) fp64 on the device, computed once per case and shared (never modified)."""
    if key not in _REF:
        o, l = shift_ref.ref_fwd(q, k, v, scale, causal, window, shift, softcap)
        _REF[key] = (o, l) + shift_ref.ref_bwd(do, q, k, v, o.to(q.dtype), l, scale, causal, window, shift, softcap)
    return _REF[key]


def _check_fwd(out, lse, ref, dt, what):
    assert_close(out, ref[0], *TOL[dt]["out"], f"{what} out")
    assert_close(lse, ref[1], *TOL[dt]["out"], f"{what} lse")


def _run_fwd(q, k, v, scale, causal, window, shift, **kw):
    from yunchang_amd import _C
    out = torch.full_like(q, float("nan"))
    lse = torch.full((q.shape[0], q.shape[2], q.shape[1]), float("nan"), dtype=torch.float32, device=q.device)
    _C.flash_fwd(q, k, v, scale, causal, lse, out=out, window=window, shift=shift, **kw)
    return out, lse, _C.last_launch_kinds()


def _run_bwd(do, q, k, v, ref, scale, causal, window, shift, only=None, **kw):
    from yunchang_amd import _C
    out16 = ref[0].to(q.dtype)
    lse = ref[1].to(torch.float32)
    delta = torch.empty_like(lse)
    _C.bwd_delta(do, out16, delta)
    dq, dk, dv = (torch.full(t.shape, float("nan"), dtype=torch.float32, device=q.device) for t in (q, k, v))
    _C.flash_bwd(do, q, k, v, lse, delta, dq, dk, dv, scale, causal, window=window, shift=shift, only=only, **kw)
    return (dq, dk, dv), _C.last_launch_kinds()


# ---- 1. block kernels with a shift ----------------------------------------------------------------------------------------------------
C = 320           # ragged against the 64-key tile, the 128-key dK/dV block and the 256-row item
SHIFTED = [(320, False, (40, -1)), (320, False, (327, -1)), (640, False, (700, -1)), (0, True, (40, 0)), (-320, False, (-1, 330)),
           (-320, False, (500, 400)), (320, True, None), (-100, True, None), (-700, True, None),          # causal_off < -Sq: every row
           (960, False, (40, -1))]                                              # empty through the right bound; the last: through the left
NO_LEFT = [c for c in SHIFTED if c[2] is None or c[2][0] < 0]
BLOCK_CASES = [("wave32", D, dt, c) for D in (128, 64) for dt in ("bfloat16", "float16") for c in SHIFTED] + \
              [("row64", 128, dt, c) for dt in ("bfloat16", "float16") for c in NO_LEFT]


@pytest.mark.parametrize("family,D,dt,case", BLOCK_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_block_kernels_with_a_shift(dev, family, D, dt, case):
    shift, causal, window = case
    q, k, v, do = _case(dev, 2, C, C, 4, 2, D, dt, seed=1)
    scale = D ** -0.5
    ref = _reference(("blk", D, dt, case), q, k, v, do, scale, causal, window, shift)
    what = f"{family} D{D} {dt} shift {shift} causal {causal} window {window}"
    out, lse, kinds = _run_fwd(q, k, v, scale, causal, window, shift, family=family)
    if family == "row64":
        assert kinds == ("fwd_row64",), kinds
    _check_fwd(out, lse, ref, dt, what)
    if case in SHIFTED[-2:]:
        assert bool((out == 0).all()) and bool(torch.isinf(lse).all()) and bool((lse < 0).all())
    for heads in (1, 2):
        grads, kinds = _run_bwd(do, q, k, v, ref, scale, causal, window, shift, family=family, dkdv_heads=heads)
        if family == "row64":
            assert "dkdv_row64" in kinds and "dq_row64" in kinds, kinds
        for g, r, name in zip(grads, ref[2:], ("dq", "dk", "dv")):
            assert_close(g, r, *grad_tol(dt, 2), f"{what} heads {heads} {name}")
        if case in SHIFTED[-2:]:
            assert all(bool((g == 0).all()) for g in grads)


@pytest.mark.parametrize("D,dt", [(128, "bfloat16"), (64, "float16")])
def test_shifted_block_with_unequal_lengths_merge_and_single_launches(dev, D, dt):
    """Sq != Sk (200 x 320) with a shift; the forward merged into a running result with a partial final range; the backward's two
    launches one at a time."""
    from yunchang_amd import _C
    Sq, Sk, shift, causal, window = 200, 320, 70, False, (90, 25)
    q, k, v, do = _case(dev, 2, Sq, Sk, 4, 2, D, dt, seed=2)
    scale = D ** -0.5
    ref = _reference(("uneq", D, dt), q, k, v, do, scale, causal, window, shift)
    out, lse, _ = _run_fwd(q, k, v, scale, causal, window, shift, family="wave32")
    _check_fwd(out, lse, ref, dt, "200x320")
    # two key halves: the first adopts, the second merges; rows [50, 150) are final in the second launch
    acc = torch.full(q.shape, float("nan"), dtype=torch.float32, device=dev)
    out2 = torch.full_like(q, float("nan"))
    lse2 = torch.full_like(lse, float("nan"))
    h = 192
    _C.flash_fwd(q, k[:, :h], v[:, :h], scale, causal, lse2, out=out2, acc=acc, final_end=0, window=window,
                 shift=shift + (Sk - h), family="wave32")                  # (bottom-right alignment: Sk - Sq changes with the cut)
    _C.flash_fwd(q, k[:, h:], v[:, h:], scale, causal, lse2, out=out2, acc=acc, merge_in=True, final_begin=50, final_end=150,
                 window=window, shift=shift, family="wave32")              # (the trailing keys keep the alignment)
    assert_close(lse2, ref[1], *TOL[dt]["out"], "merged lse")
    assert_close(out2[:, 50:150], ref[0][:, 50:150], *TOL[dt]["out"], "merged out, final rows")
    assert_close(torch.cat([acc[:, :50], acc[:, 150:]], 1), torch.cat([ref[0][:, :50], ref[0][:, 150:]], 1), *TOL[dt]["out"],
                 "merged out, running rows")
    (dq, dk, dv), kinds = _run_bwd(do, q, k, v, ref, scale, causal, window, shift, only="dq", family="wave32")
    assert kinds == ("dq_wave8",) and bool(torch.isnan(dk).all()) and bool(torch.isnan(dv).all())
    assert_close(dq, ref[2], *grad_tol(dt), "only dq")
    (dq, dk, dv), kinds = _run_bwd(do, q, k, v, ref, scale, causal, window, shift, only="dkdv", family="wave32")
    assert "dkdv_wave8" in kinds and "dq_wave8" not in kinds and bool(torch.isnan(dq).all())
    assert_close(dk, ref[3], *grad_tol(dt, 2), "only dkdv: dk")
    assert_close(dv, ref[4], *grad_tol(dt, 2), "only dkdv: dv")


# ---- 2. windowed launches with left-cut, interior and right-cut tiles in every 256-row item ---------------------------------
WINDOWS = [((448, 0), True), ((300, 200), False), ((70, -1), False)]


@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("window,causal", WINDOWS, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("Sk,shift", [(1024, None), (1280, 256)])
def test_windowed_forward_tile_order(dev, D, window, causal, Sk, shift):
    """Against the exact reference, and against the same launch with softcap = 1e4 (tanh is the identity to 1e-9 there): that
    launch runs the softcap instantiation, which sends every tile through the generic loop in ascending order, while the window
    instantiation walks the tiles rotated and its interior tiles in the pipelined loop.  Agreement pins the new order."""
    dt = "bfloat16"
    q, k, v, do = _case(dev, 1, 1024, Sk, 2, 1, D, dt, seed=3)
    scale = D ** -0.5
    ref = _reference(("tiles", D, window, Sk), q, k, v, do, scale, causal, window, shift or 0)
    for n in (0, 2):
        out, lse, kinds = _run_fwd(q, k, v, scale, causal, window, shift, family="wave32", k_splits=n)
        assert ("fwd_split_merge" in kinds) == (n == 2), kinds
        _check_fwd(out, lse, ref, dt, f"D{D} {window} k_splits {n}")
        out_c, lse_c, _ = _run_fwd(q, k, v, scale, causal, window, shift, family="wave32", k_splits=n, softcap=1e4)
        assert_close(out, out_c.double(), *TOL[dt]["out"], f"D{D} {window} k_splits {n}: out vs the generic loop")
        assert_close(lse, lse_c.double(), *TOL[dt]["out"], f"D{D} {window} k_splits {n}: lse vs the generic loop")


# ---- 3. virtual ranks on one GPU --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nccl_single():
    import torch.distributed as dist
    import yunchang_amd  # noqa: F401
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29735")
    own = not dist.is_initialized()
    if own:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    yield dist
    if own:
        dist.destroy_process_group()


def _virtual_run(monkeypatch, nccl_single, dev, ud, rd, c, window, causal, softcap=0.0, repeat_backward=False, inputs=None):
    """Every rank of a ud x rd grid as a thread: Ulysses exchange by hand (autograd cannot run the ranks' backwards side by
    side), the ring forward and backward of the package with the real HipBlockBackend.  Returns per rank (out, dq, dk, dv
    [, dk, dv of a second backward]) and the unsharded inputs (`inputs`: S -> (q, k, v, do) in place of the N(0,1) draw)."""
    import yunchang_amd.comm.all_to_all as A
    import yunchang_amd.ring.ring_flash_attn as R
    from yunchang_amd.kernels import get_block_backend
    from virtual_grid import VirtualGridPairwise, patch_dist, run_grid
    assert get_block_backend().name == "hip"
    monkeypatch.setenv("USP_RING_WINDOW", "global")
    grid = VirtualGridPairwise(ud, rd, nccl_single)
    patch_dist(monkeypatch, grid)
    ws, Hq, Hkv, D = ud * rd, 4, 2, 128
    S = c * rd
    q, k, v, do = _case(dev, 1, S, S, Hq, Hkv, D, "bfloat16", seed=4) if inputs is None else inputs(S)
    rows = S // ws
    loc = [[t[:, r * rows:(r + 1) * rows].contiguous() for t in (q, k, v, do)] for r in range(ws)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(ws)]
    scale = D ** -0.5
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        upg, rpg = grid.groups_of(r)
        lq, lk, lv, ldo = loc[r]
        with torch.cuda.stream(streams[r]):
            hq, hdo = (A.heads_to_seq(t, upg, contiguous=True) for t in (lq, ldo))
            hk, hv = (A.kv_heads_to_seq(t, upg, contiguous=True) for t in (lk, lv))
            out, lse = R.ring_flash_attn_forward(rpg, hq, hk, hv, scale, causal=causal, window_size=window, softcap=softcap)
            res = []
            for _ in range(2 if repeat_backward else 1):
                dq, dk, dv = R.ring_flash_attn_backward(rpg, hdo, hq, hk, hv, out, lse, scale, causal=causal, window_size=window,
                                                        softcap=softcap)
                res += [A.kv_seq_to_heads(dk, upg, Hkv), A.kv_seq_to_heads(dv, upg, Hkv)]
            return [A.seq_to_heads(out, upg), A.seq_to_heads(dq, upg)] + res
    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    return res, (q, k, v, do), rows, scale


VIRTUAL = [(2, 2, (40, 0), True, 0.0), (2, 2, (700, 0), True, 0.0), (1, 4, (40, 0), True, 0.0), (1, 4, (400, 0), True, 0.0), (1, 4, (700, 0), True, 0.0), (1, 4, (100, 60), False, 0.0),
           (1, 4, (400, 0), True, 30.0), (2, 2, (400, 0), True, 0.0), (2, 2, (100, 60), False, 0.0)]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("ud,rd,window,causal,softcap", VIRTUAL, ids=lambda v: str(v).replace(" ", ""))
def test_global_window_on_virtual_ranks(dev, nccl_single, monkeypatch, ud, rd, window, causal, softcap):
    c = 320 if rd == 4 else 640
    twice = (ud, rd, window) == (1, 4, (400, 0)) and not softcap
    res, (q, k, v, do), rows, scale = _virtual_run(monkeypatch, nccl_single, dev, ud, rd, c, window, causal, softcap, twice)
    ref = _reference(("virtual", rd * c, window, softcap), q, k, v, do, scale, causal, window, 0, softcap or None)
    for r in range(ud * rd):
        sl = slice(r * rows, (r + 1) * rows)
        what = f"{ud}x{rd} window {window} rank {r}"
        assert_close(res[r][0], ref[0][:, sl], *TOL["bfloat16"]["out"], f"{what} out")
        for got, want, name in zip(res[r][1:4], (ref[2], ref[3], ref[4]), ("dq", "dk", "dv")):
            assert_close(got, want[:, sl], *grad_tol("bfloat16", 2), f"{what} {name}")
        if twice:
            assert torch.equal(res[r][2], res[r][4]) and torch.equal(res[r][3], res[r][5]), f"{what}: dk / dv of two identical calls"


RING_NEEDLE = [(ud, rd, w, causal) for ud, rd in ((1, 4), (2, 2))
               for w, causal in (("c-1", True), ("c", True), ("c+1", True), ((100, 60), False))]


def ring_needle_inputs(S, c, window, causal, Hq=4, Hkv=2, D=128, dt="bfloat16"):
    """Needle inputs (tests/needle_inputs.py) over the GLOBAL sequence of a ring of chunks of c rows: private needles on the
    mask edges of sampled global rows and of the last / first row of every rank block, and on the last key of a block and the
    first of the next for rows that see both."""
    import needle_inputs as NI
    import test_gpu_needle as GN
    rows = sorted(set(NI.sample_rows(S, 10, 3)) | {r for m in range(1, S // c) for r in (m * c - 1, m * c)})
    edges = NI.mask_edges(rows, S, S, causal, window)
    for kb in range(c, S, c):
        for r in (kb + 9, min(S - 1, kb + c - 1)):
            if all(NI._visible(r, j, S, S, causal, window) for j in (kb - 1, kb)):
                edges += [(r, kb - 1), (r, kb)]
    C = GN.classes_for(GN._keys_seen(S, S, causal, window), D)
    return NI.make(S, S, Hq, Hkv, D, dt, C, seed=90, edges=edges)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("ud,rd,w,causal", RING_NEEDLE, ids=lambda v: str(v).replace(" ", ""))
def test_global_window_on_virtual_ranks_with_needle_inputs(dev, nccl_single, monkeypatch, ud, rd, w, causal):
    """The same ring runs on needle inputs, at the windows where the planner's empty / `keys` / `rows` decisions flip (c - 1, c,
    c + 1: the block two ranks back holds no, no, one visible (row, key) pair), judged per rank with `needle_inputs.verdicts`
    against the GLOBAL fp64 reference: a ring block that loses or adds the one key on a bound is a 100 % error on a sampled row."""
    import needle_inputs as NI
    c = 320 if rd == 4 else 640
    window = {"c-1": (c - 1, 0), "c": (c, 0), "c+1": (c + 1, 0)}.get(w, w)
    made = {}

    def inputs(S):
        made["nd"] = nd = ring_needle_inputs(S, c, window, causal)
        return [torch.from_numpy(x).to(torch.bfloat16).to(dev) for x in (nd.q, nd.k, nd.v, nd.do)]
    res, (q, k, v, do), rows, scale = _virtual_run(monkeypatch, nccl_single, dev, ud, rd, c, window, causal, inputs=inputs)
    S = q.shape[1]
    ref = _reference(("needle", ud, rd, window), q, k, v, do, scale, causal, window, 0)
    for r in range(ud * rd):
        sl = slice(r * rows, (r + 1) * rows)
        got = dict(zip(("out", "dq", "dk", "dv"), res[r][:4]))
        want = {n_: t[:, sl] for n_, t in zip(("out", "dq", "dk", "dv"), (ref[0], ref[2], ref[3], ref[4]))}
        ver = NI.verdicts(got, want, "bfloat16", S, S, 2)
        print(f"[needle-ring] {ud}x{rd} window {window} rank {r}: " + " ".join(f"{n_}={x:.3f}" for n_, (_, x) in ver.items()))
        bad = {n_: round(x, 3) for n_, (ok, x) in ver.items() if not ok}
        assert not bad, f"{ud}x{rd} window {window} rank {r}: out of tolerance, worst error / bound {bad}"


# ---- 4. two processes sharing the GPU ------------------------------------------------------------------------------------------
def _two_process_worker(rank, ws):
    """(RCCL refuses two ranks on one device: the transport is gloo, ordered like RCCL, as in tests/test_gpu_multiproc.py.)"""
    import yunchang_amd as Y
    from test_gpu_multiproc import _order_p2p_like_rccl
    from yunchang_amd.kernels import get_block_backend
    _order_p2p_like_rccl()
    assert get_block_backend().name == "hip"
    os.environ["USP_RING_WINDOW"] = "global"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    Y.set_seq_parallel_pg(1, ws, rank, ws)
    q, k, v, do = _case(torch.device("cpu"), 2, 640, 640, 4, 2, 128, "bfloat16", seed=6)
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    lq, lk, lv, ldo = (ext(t, rank, world_size=ws, rd=ws, ud=1).detach().clone().to(dev) for t in (q, k, v, do))
    for t in (lq, lk, lv):
        t.requires_grad_(True)
    out = Y.LongContextAttention(ring_impl_type="basic", attn_type=Y.AttnType.HIP)(lq, lk, lv, causal=True, window_size=(100, 0))
    out.backward(ldo)
    torch.cuda.synchronize()
    ref = shift_ref.ref_fwd(q, k, v, 128 ** -0.5, True, (100, 0))
    ref = ref[:1] + shift_ref.ref_bwd(do, q, k, v, ref[0].to(torch.bfloat16), ref[1], 128 ** -0.5, True, (100, 0))
    truth = [ext(t, rank, world_size=ws, rd=ws, ud=1) for t in ref]
    return [t.detach().double().cpu() for t in (out, lq.grad, lk.grad, lv.grad)], truth


@pytest.mark.timeout(300)
def test_global_window_two_processes_one_gpu():
    for rank, (got, truth) in enumerate(run_distributed(_two_process_worker, 2)):
        for a, t, name in zip(got, truth, ("out", "dq", "dk", "dv")):
            tol = TOL["bfloat16"]["out"] if name == "out" else grad_tol("bfloat16", 2)
            assert_close(a, t, *tol, f"two processes, rank {rank}: {name}")


# ---- 5. extreme window bounds and shifts: everything or nothing visible -----------------------------------------------------------------
_IMAX, _SMAX = (1 << 31) - 1, (1 << 30) - 1
# (causal, window, shift, what the mask leaves: "all" | "none" | "causal", a left bound that cuts -> not for the 64-row family)
EXTREME = [(False, (_IMAX, -1), None, "all", False), (False, (-1, _IMAX), None, "all", False), (True, (_IMAX, 0), None, "causal", False),
           (False, (_IMAX, _IMAX), None, "all", False), (False, (_IMAX, -1), _SMAX, "all", False), (False, (_IMAX, -1), -_SMAX, "all", False),
           (False, (-1, _IMAX), _SMAX, "all", False), (False, (-1, _IMAX), -_SMAX, "all", False), (False, (_IMAX, _IMAX), -_SMAX, "all", False),
           (True, None, _SMAX, "all", False), (True, None, -_SMAX, "none", False), (True, (_IMAX, 0), -_SMAX, "none", False),
           (False, (5, -1), _SMAX, "none", True), (False, (-1, 5), -_SMAX, "none", False), (False, (_IMAX, 5), _SMAX, "all", False)]


@pytest.mark.parametrize("Sq,Sk", [(320, 320), (200, 320), (320, 200)])
def test_extreme_window_bounds_and_shifts(dev, Sq, Sk):
    """window_left / window_right = INT32_MAX (a caller's "unbounded"), alone and with a shift of +-(2^30 - 1), where the result
    is every key, no key, or plain causal: both families and the default dispatch against tests/shift_ref.py at the stated
    tolerances; an empty result is exactly out = 0, lse = -inf, zero gradients.  (The host decode of these values is swept on
    the CPU first, tests/test_host_api.py: the sums are formed in 64 bits, a bound that cuts nothing is dropped -- which is what
    lets the 64-row family take a call whose left bound is INT32_MAX.)"""
    dt, D = "bfloat16", 128
    q, k, v, do = _case(dev, 2, Sq, Sk, 4, 2, D, dt, seed=7)
    scale = D ** -0.5
    for causal, window, shift, left_over, left_cuts in EXTREME:
        vis = shift_ref.visible(Sq, Sk, causal, window, shift or 0)
        plain = shift_ref.visible(Sq, Sk, left_over == "causal")
        assert torch.equal(vis, plain if left_over != "none" else torch.zeros_like(vis)), (causal, window, shift)
        ref = _reference(("extreme", Sq, Sk, causal, window, shift), q, k, v, do, scale, causal, window, shift or 0)
        for family in ("row64", "wave32", None):
            if family == "row64" and left_cuts:
                continue
            what = f"{Sq}x{Sk} causal {causal} window {window} shift {shift} family {family}"
            out, lse, kinds = _run_fwd(q, k, v, scale, causal, window, shift, family=family)
            if family == "row64":
                assert kinds == ("fwd_row64",), (what, kinds)
            _check_fwd(out, lse, ref, dt, what)
            grads, kinds = _run_bwd(do, q, k, v, ref, scale, causal, window, shift, family=family)
            if family == "row64":
                assert "dkdv_row64" in kinds and "dq_row64" in kinds, (what, kinds)
            for g, r, name in zip(grads, ref[2:], ("dq", "dk", "dv")):
                assert_close(g, r, *grad_tol(dt, 2), f"{what} {name}")
            if left_over == "none":
                assert bool((out == 0).all()) and bool(torch.isinf(lse).all()) and bool((lse < 0).all()), what
                assert all(bool((g == 0).all()) for g in grads), what


def test_python_entry_points_pass_an_int32_max_window_through(dev):
    """hip_attn_forward / hip_attn_backward / hip_attn_func with window_size = (2^31 - 1, 0), causal: the unwindowed causal result."""
    from yunchang_amd.kernels.attention import hip_attn_backward, hip_attn_forward, hip_attn_func
    dt = "bfloat16"
    q, k, v, do = _case(dev, 1, 320, 200, 4, 2, 128, dt, seed=8)
    win = ((1 << 31) - 1, 0)
    out0, lse0 = hip_attn_forward(q, k, v, causal=True)
    out1, lse1 = hip_attn_forward(q, k, v, causal=True, window_size=win)
    assert_close(out1, out0.double(), *TOL[dt]["out"], "hip_attn_forward out")
    assert_close(lse1, lse0.double(), *TOL[dt]["out"], "hip_attn_forward lse")
    g0, g1 = ([torch.full_like(t, float("nan")) for t in (q, k, v)] for _ in range(2))
    hip_attn_backward(do, q, k, v, out0, lse0, *g0, bwd_causal=True)
    hip_attn_backward(do, q, k, v, out0, lse0, *g1, bwd_causal=True, window_size=win)
    for a, b, name in zip(g1, g0, ("dq", "dk", "dv")):
        assert_close(a, b.double(), *grad_tol(dt, 2), f"hip_attn_backward {name}")
    res = []
    for w in ((-1, -1), win):
        leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
        o = hip_attn_func(*leaves, causal=True, window_size=w)
        o.backward(do)
        res.append([o.detach()] + [t.grad for t in leaves])
    for a, b, name in zip(res[1], res[0], ("out", "dq", "dk", "dv")):
        assert_close(a, b.double(), *(TOL[dt]["out"] if name == "out" else grad_tol(dt, 2)), f"hip_attn_func {name}")
