"""The document mask (cu_doclens) on the GPU: the document instantiations of the two-waves-per-SIMD kernels (usp_flash_fwd_doc /
usp_flash_bwd_doc) against tests/doc_ref.py (fp64, on the device) on needle inputs on which one boundary moved by one key is an
O(1) error (tests/test_doc_mask_cpu.py::test_boundary_mutants_fail shows that with the reference alone); bit-identity with the
plain launches; launch kinds and refusals; hip_attn_func and LongContextAttention at a padded head dim; the basic ring on
virtual ranks; eight documents in one sequence against a batch of eight.

Shapes: Sq = Sk in {320, 1280} -- 320 is ragged against the 128-key dK/dV block and the 128 / 256-row items, 1280 is several of
each -- with boundaries on, one before and one after multiples of 64, a run of ten documents of length 1, one document of 700
(interior tiles take the pipelined loop) and the full block of a ring below the diagonal (256 rows against 512 earlier keys,
rows with row_lo = Sk included)."""
import ctypes

import numpy as np
import pytest
import torch

import doc_ref
import needle_inputs
from golden_util import TOL, assert_close, grad_tol

pytestmark = pytest.mark.gpu

CU = {320: [0, 63, 64, 65, 96, 128, 255, 256, 257, 320],
      1280: [0, 63, 64, 65, 96, 128, 255, 256, 257] + list(range(300, 311)) + [1010, 1280]}
_WAVE_FWD = {"fwd_wave8", "fwd_wave4"}
_WAVE_BWD = {"dkdv_wave8", "dq_wave8", "reduce_heads"}


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _arrays(dev, cu, row0, n_rows, key0, n_keys):
    from yunchang_amd.ring import doc_blocks
    rl, kh = doc_blocks.block_arrays(cu, row0, n_rows, key0, n_keys)
    return torch.from_numpy(rl).to(dev), torch.from_numpy(kh).to(dev), rl


_IN, _REF = {}, {}


def _inputs(dev, S, Hq, Hkv, D, dt):
    """Needle inputs of the diagonal case (tests/doc_ref.py: needle_edges), once per shape."""
    key = (S, Hq, Hkv, D, dt)
    if key not in _IN:
        nd = needle_inputs.make(S, S, Hq, Hkv, D, dt, C=8, seed=S + D, edges=doc_ref.needle_edges(CU[S], S))
        _IN[key] = [torch.from_numpy(x.astype(np.float32)).to(getattr(torch, dt)).to(dev) for x in (nd.q, nd.k, nd.v, nd.do)]
    return _IN[key]


def _reference(key, do, q, k, v, scale, mask):
    if key not in _REF:
        _REF[key] = doc_ref.ref_bwd(do, q, k, v, scale, mask, out_dtype=q.dtype)
    return _REF[key]


def _fwd(q, k, v, scale, causal, doc, **kw):
    from yunchang_amd import _C
    out = torch.full_like(q, float("nan"))
    lse = torch.full((q.shape[0], q.shape[2], q.shape[1]), float("nan"), dtype=torch.float32, device=q.device)
    _C.flash_fwd(q, k, v, scale, causal, lse, out=out, doc=doc, **kw)
    return out, lse, _C.last_launch_kinds()


def _bwd(do, q, k, v, ref, scale, causal, doc, **kw):
    from yunchang_amd import _C
    lse = ref[1].to(torch.float32)
    delta = torch.empty_like(lse)
    _C.bwd_delta(do, ref[0].to(q.dtype), delta)
    dq, dk, dv = (torch.full(t.shape, float("nan"), dtype=torch.float32, device=q.device) for t in (q, k, v))
    _C.flash_bwd(do, q, k, v, lse, delta, dq, dk, dv, scale, causal, doc=doc, **kw)
    return (dq, dk, dv), _C.last_launch_kinds()


def _check(out, lse, grads, ref, dt, G, what):
    assert_close(out, ref[0], *TOL[dt]["out"], f"{what} out")
    assert_close(lse, ref[1], 2e-3, 1e-4, f"{what} lse")
    for g, r, name in zip(grads, ref[2:], ("dq", "dk", "dv")):
        assert_close(g, r, *grad_tol(dt, G), f"{what} {name}")


# ---- 1. kernel parity, causal launches ----------------------------------------------------------------------------------------
PARITY = [(dt, D, 4, 1, 0, S) for dt in ("bfloat16", "float16") for D in (32, 64, 128) for S in (320, 1280)] + \
         [("bfloat16", 64, 1, 1, 0, 320), ("float16", 128, 1, 1, 0, 1280), ("bfloat16", 128, 4, 1, 1, 320), ("float16", 64, 4, 1, 1, 1280),
          ("bfloat16", 64, 4, 4, 0, 320)]


@pytest.mark.parametrize("dt,D,Hq,Hkv,dkdv_heads,S", PARITY, ids=lambda v: str(v))
def test_kernel_parity_causal(dev, dt, D, Hq, Hkv, dkdv_heads, S):
    q, k, v, do = _inputs(dev, S, Hq, Hkv, D, dt)
    scale = D ** -0.5
    rl, kh, _ = _arrays(dev, CU[S], 0, S, 0, S)
    ref = _reference(("diag", dt, D, Hq, Hkv, S), do, q, k, v, scale, doc_ref.global_mask(CU[S], S))
    out, lse, kinds = _fwd(q, k, v, scale, True, (rl, kh))
    assert kinds and set(kinds) <= _WAVE_FWD, kinds
    grads, kinds = _bwd(do, q, k, v, ref, scale, True, (rl, kh), dkdv_heads=dkdv_heads)
    assert {"dkdv_wave8", "dq_wave8"} <= set(kinds) <= _WAVE_BWD, kinds
    _check(out, lse, grads, ref, dt, Hq // Hkv, f"{dt} D{D} H{Hq}/{Hkv} heads/item {dkdv_heads} S{S}")


# ---- 2. the ring's block below the diagonal: a full launch with a left bound, merge_in with acc, interleave -----------------------------
OFFDIAG_CU, OFFDIAG_ROW0 = [0, 200, 449, 520, 768], 512


def offdiag_inputs(dt, D):
    """The ring's block below the diagonal, host arrays: rows = global [512, 768), keys = global [0, 512); documents end at 200,
    449, 520 (rows from 520 on see nothing: row_lo = Sk).  Needles on the last hidden and the first visible key (448, 449) for
    the block's rows 0, 1 and 7 -- the boundary 449 moved by one key is an O(1) error -- and on key 449 for row 8, the first row
    that sees nothing: the boundary 520 moved by one row empties row 7 or fills row 8
    (tests/test_doc_mask_cpu.py::test_offdiagonal_mutants_fail)."""
    edges = [(r, j) for r in (0, 1, 7) for j in (448, 449)] + [(8, 449)]
    return needle_inputs.make(256, 512, 4, 1, D, dt, C=8, seed=5 + D, edges=edges)


def _offdiag(dev, dt, D):
    nd = offdiag_inputs(dt, D)
    t = [torch.from_numpy(x.astype(np.float32)).to(getattr(torch, dt)).to(dev) for x in (nd.q, nd.k, nd.v, nd.do)]
    return OFFDIAG_CU, t


@pytest.mark.parametrize("dt,D", [("bfloat16", 128), ("float16", 64), ("bfloat16", 32)], ids=lambda v: str(v))
@pytest.mark.parametrize("mode", ["plain", "merge_in", "interleave"])
def test_full_block_with_left_bound(dev, dt, D, mode):
    from yunchang_amd import _C
    cu, (q, k, v, do) = _offdiag(dev, dt, D)
    Sq, Sk = q.shape[1], k.shape[1]
    rl, kh, rl_host = _arrays(dev, cu, OFFDIAG_ROW0, Sq, 0, Sk)
    assert rl_host.max() == Sk and rl_host.min() == 449          # rows that see nothing are in the launch
    scale = D ** -0.5
    mask = doc_ref.block_mask(rl_host, Sq, Sk, False)
    ref = doc_ref.ref_bwd(do, q, k, v, scale, mask, out_dtype=q.dtype)
    what = f"{dt} D{D} {mode}"
    if mode == "merge_in":
        # the running state of the rows: a first block over other keys (plain full launch), then this block merged in, to acc
        g = torch.Generator().manual_seed(3)
        k0, v0 = (torch.randn(1, 128, 1, D, generator=g).to(q.dtype).to(dev) for _ in range(2))
        acc = torch.empty(q.shape, dtype=torch.float32, device=dev)
        lse = torch.empty((1, 4, Sq), dtype=torch.float32, device=dev)
        out = torch.full_like(q, float("nan"))
        _C.flash_fwd(q, k0, v0, scale, False, lse, out=out, acc=acc, final_begin=0, final_end=0, family="wave32")
        _C.flash_fwd(q, k, v, scale, False, lse, out=out, acc=acc, merge_in=True, final_begin=0, final_end=100, doc=(rl, kh))
        m2 = torch.cat([torch.ones(1, Sq, 128, dtype=torch.bool), mask], dim=2)
        want = doc_ref.ref_fwd(q, torch.cat([k0, k], 1), torch.cat([v0, v], 1), scale, m2)
        assert_close(out[:, :100], want[0][:, :100], *TOL[dt]["out"], f"{what} out (final rows)")
        assert_close(acc[:, 100:], want[0][:, 100:], *TOL[dt]["out"], f"{what} acc (the other rows)")
        assert_close(lse, want[1], 2e-3, 1e-4, f"{what} lse")
        return
    kw = dict(interleave=True) if mode == "interleave" else {}
    out, lse, kinds = _fwd(q, k, v, scale, False, (rl, kh), **kw)
    assert kinds and set(kinds) <= _WAVE_FWD, kinds
    empty = torch.from_numpy(rl_host == Sk).to(dev)
    assert bool((out[0, empty] == 0).all()) and bool(torch.isneginf(lse[0, :, empty]).all()), "rows that see nothing: out = 0, lse = -inf"
    grads, kinds = _bwd(do, q, k, v, ref, scale, False, (rl, kh), **kw)
    assert bool((grads[0][0, empty] == 0).all()), "rows that see nothing: dq = 0"
    _check(out, lse, grads, ref, dt, 4, what)


# ---- 3. every tensor in a strided layout of its own ---------------------------------------------------------------------------------
def test_independent_layouts(dev):
    from layout_util import Arena, blank, draw_layout, place
    from yunchang_amd import _C
    dt, D, S = "bfloat16", 64, 320
    q, k, v, do = _inputs(dev, S, 4, 1, D, dt)
    scale = D ** -0.5
    rl, kh, _ = _arrays(dev, CU[S], 0, S, 0, S)
    ref = _reference(("diag", dt, D, 4, 1, S), do, q, k, v, scale, doc_ref.global_mask(CU[S], S))
    rs = np.random.RandomState(11)
    arena = Arena(dev)
    pq, pk, pv, pdo = (place(t, draw_layout(rs, "in16", 1), arena, n) for t, n in ((q, "q"), (k, "k"), (v, "v"), (do, "dout")))
    out = blank(q.shape, q.dtype, draw_layout(rs, "out16", 1), arena, "out")
    lse = blank((1, 4, S), torch.float32, draw_layout(rs, "lse", 1), arena, "lse")
    _C.flash_fwd(pq, pk, pv, scale, True, lse, out=out, doc=(rl, kh))
    delta = blank((1, 4, S), torch.float32, draw_layout(rs, "lse", 1), arena, "delta")
    plse = place(ref[1].to(torch.float32), draw_layout(rs, "lse", 1), arena, "lse_in")
    _C.bwd_delta(pdo, place(ref[0].to(q.dtype), draw_layout(rs, "in16", 1), arena, "o"), delta)
    dq, dk, dv = (blank(t.shape, torch.float32, draw_layout(rs, "f32", 1), arena, n) for t, n in ((q, "dq"), (k, "dk"), (v, "dv")))
    _C.flash_bwd(pdo, pq, pk, pv, plse, delta, dq, dk, dv, scale, True, doc=(rl, kh))
    torch.cuda.synchronize()
    assert arena.untouched(), arena.violations()
    assert arena.unchanged()
    _check(out, lse, (dq, dk, dv), ref, dt, 4, "independent layouts")


# ---- 4. bit-identity: NULL arrays and the single document are the plain wave32 launch ------------------------------------------------
@pytest.mark.parametrize("D,S", [(128, 1280), (64, 320)])
def test_bit_identity_with_the_plain_family(dev, D, S):
    dt = "bfloat16"
    q, k, v, do = _inputs(dev, S, 4, 1, D, dt)
    scale = D ** -0.5
    ref = _reference(("diag", dt, D, 4, 1, S), do, q, k, v, scale, doc_ref.global_mask(CU[S], S))
    plain_f = _fwd(q, k, v, scale, True, None, family="wave32")
    plain_b = _bwd(do, q, k, v, ref, scale, True, None, family="wave32", splits=(0, 0))
    one = (torch.zeros(S, dtype=torch.int32, device=dev), torch.full((S,), S, dtype=torch.int32, device=dev))
    for doc, what in ((one, "single document"), ((None, None), "NULL arrays")):
        f = _fwd(q, k, v, scale, True, doc, family="wave32")
        b = _bwd(do, q, k, v, ref, scale, True, doc, family="wave32", splits=(0, 0))
        for a, c, name in zip(f[:2] + b[0], plain_f[:2] + plain_b[0], ("out", "lse", "dq", "dk", "dv")):
            assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                               c.view(torch.int32 if c.dtype == torch.float32 else torch.int16)), f"{what}: {name} differs in bits"


# ---- 5. refusals on the device: nothing launched, nothing written ------------------------------------------------------------------
def test_refusals_launch_nothing(dev):
    from yunchang_amd import _C
    D, S = 64, 320
    q, k, v, do = _inputs(dev, S, 4, 1, D, "bfloat16")
    rl, kh, _ = _arrays(dev, CU[S], 0, S, 0, S)
    for kw in (dict(window=(16, 0)), dict(softcap=30.0), dict(shift=0), dict(family="row64")):
        out = torch.full_like(q, 7.0)
        lse = torch.full((1, 4, S), 7.0, dtype=torch.float32, device=dev)
        with pytest.raises(RuntimeError, match="not supported|unsupported"):
            _C.flash_fwd(q, k, v, D ** -0.5, True, lse, out=out, doc=(rl, kh), **kw)
        torch.cuda.synchronize()
        assert _C.last_launch_kinds() == () and bool((out == 7.0).all()) and bool((lse == 7.0).all()), kw
        g = [torch.full(t.shape, 7.0, dtype=torch.float32, device=dev) for t in (q, k, v)]
        with pytest.raises(RuntimeError, match="not supported|unsupported"):
            _C.flash_bwd(do, q, k, v, lse, lse, *g, D ** -0.5, True, doc=(rl, kh), **kw)
        torch.cuda.synchronize()
        assert _C.last_launch_kinds() == () and all(bool((t == 7.0).all()) for t in g), kw
    # a packed batch: the binding's packed calls take no `doc`, so the argument blocks are filled here as flash_fwd_packed /
    # flash_bwd_packed fill them (token tensors (T, H, D), lse (H, T), one sequence of S tokens) and handed to the entry points
    tq, tk, tv, tdo = (t[0] for t in (q, k, v, do))
    seq = torch.tensor([[0, S]], dtype=torch.int32, device=dev)
    out = torch.full_like(tq, 7.0)
    lse = torch.full((4, S), 7.0, dtype=torch.float32, device=dev)
    g = [torch.full(t.shape, 7.0, dtype=torch.float32, device=dev) for t in (tq, tk, tv)]
    a = _C.UspFwdArgs()
    b = _C.UspBwdArgs()
    for x in (a, b):
        x.dtype, x.B, x.Sq, x.Sk, x.Hq, x.Hkv, x.D, x.causal, x.softmax_scale = _C.USP_BF16, 1, S, S, 4, 1, D, 1, D ** -0.5
        x.q, x.k, x.v = _C._t3(tq), _C._t3(tk), _C._t3(tv)
        x.lse, x.lse_stride_b, x.lse_stride_h = _C._lse2(lse)
        x.seq_q = x.seq_k = seq.data_ptr()
        x.sched = _C.sched_block(dev).data_ptr()
    a.out, a.final_end = _C._t3(out), 2
    b.dout = _C._t3(tdo)
    b.delta, b.delta_stride_b, b.delta_stride_h = _C._lse2(lse)
    b.dq, b.dk, b.dv, b.total_k = _C._t3(g[0]), _C._t3(g[1]), _C._t3(g[2]), S
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert _C._doc_entry("usp_flash_fwd_doc")(ctypes.byref(a), p(rl), 0, stream) == -2
    assert _C.last_launch_kinds() == ()
    assert _C._doc_entry("usp_flash_bwd_doc")(ctypes.byref(b), p(rl), 0, p(kh), 0, stream) == -2
    assert _C.last_launch_kinds() == ()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((lse == 7.0).all()) and all(bool((t == 7.0).all()) for t in g), "packed batch"
    assert bool((_C.sched_block(dev) == 0).all()), "the queue's control block is left zeroed"


# ---- 6. the public path, at a padded head dim ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nccl_single():
    import os
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29739")
    own = not dist.is_initialized()
    if own:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    yield dist
    if own:
        dist.destroy_process_group()


@pytest.mark.parametrize("path", ["hip_attn_func", "LongContextAttention"])
def test_public_path_padded_head_dim(dev, nccl_single, path):
    import yunchang_amd as Y
    from yunchang_amd.kernels.attention import hip_attn_func
    B, S, Hq, Hkv, D, dt = 2, 320, 4, 2, 96, "bfloat16"
    g = torch.Generator().manual_seed(9)
    q, k, v, do = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv, Hq))
    cu = [CU[S], [0, 1, 100, 319, 320]]                       # one list per batch entry
    ref = doc_ref.ref_bwd(do, q, k, v, D ** -0.5, doc_ref.global_mask(cu, S, B), out_dtype=q.dtype)
    tq, tk, tv = (t.clone().requires_grad_(True) for t in (q, k, v))
    if path == "hip_attn_func":
        out = hip_attn_func(tq, tk, tv, causal=True, cu_doclens=cu)
    else:
        Y.set_seq_parallel_pg(1, 1, 0, 1)
        out = Y.LongContextAttention(ring_impl_type="basic", attn_type=Y.AttnType.HIP)(tq, tk, tv, causal=True, cu_doclens=cu)
    out.backward(do)
    _check(out, ref[1].float(), (tq.grad, tk.grad, tv.grad), ref, dt, Hq // Hkv, path)


# ---- 7. the basic ring on virtual ranks -----------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("rd", [2, 4, pytest.param((2, 2), id="ud2-rd2")])
def test_basic_ring_on_virtual_ranks(dev, nccl_single, monkeypatch, rd):
    """S_total = 1024: documents crossing rank edges, one rank (the last of four) holding only whole small documents -- its
    steps beyond the diagonal see nothing and are dropped.  (ud, rd) = (2, 2): the Ulysses exchange around the ring, built as
    tests/test_gpu_sink.py::test_grid_invariance_on_virtual_ranks builds its grid, with B = 2 and one list per entry -- a single
    document, and a list with a boundary on the ring's rank edge, so that this entry sees nothing in the second ring rank's
    step below the diagonal while the other one does."""
    import yunchang_amd.comm.all_to_all as A
    import yunchang_amd.ring.ring_flash_attn as R
    from yunchang_amd.ring import doc_blocks
    from virtual_grid import VirtualGridPairwise, patch_dist, run_grid
    ud, rd = rd if isinstance(rd, tuple) else (1, rd)
    S, Hq, Hkv, D = 1024, 4, 2, 64
    B, cu = (1, [0, 100, 300, 515, 768, 800, 900, 1024]) if ud == 1 else (2, [[0, S], [0, 100, 300, 512, 768, 800, 1024]])
    docs = doc_blocks.parse(cu, B, S)
    ws = ud * rd
    grid = VirtualGridPairwise(ud, rd, nccl_single)
    patch_dist(monkeypatch, grid)
    g = torch.Generator().manual_seed(rd if ud == 1 else 22)
    q, k, v, do = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv, Hq))
    rows, scale = S // ws, D ** -0.5
    loc = [[t[:, r * rows:(r + 1) * rows].contiguous() for t in (q, k, v, do)] for r in range(ws)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(ws)]
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        upg, rpg = grid.groups_of(r)
        lq, lk, lv, ldo = loc[r]
        with torch.cuda.stream(streams[r]):
            if ud > 1:                                       # rank = ring * ud + u: sequence shards in, head shards around the ring
                lq, ldo = (A.heads_to_seq(t, upg, contiguous=True) for t in (lq, ldo))
                lk, lv = (A.kv_heads_to_seq(t, upg, contiguous=True) for t in (lk, lv))
            out, lse = R.ring_flash_attn_forward(rpg, lq, lk, lv, scale, causal=True, cu_doclens=docs)
            grads = list(R.ring_flash_attn_backward(rpg, ldo, lq, lk, lv, out, lse, scale, causal=True, cu_doclens=docs))
            if ud > 1:
                return [A.seq_to_heads(out, upg), A.seq_to_heads(grads[0], upg), A.kv_seq_to_heads(grads[1], upg, Hkv),
                        A.kv_seq_to_heads(grads[2], upg, Hkv)]
            return [out] + grads
    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    ref = doc_ref.ref_bwd(do, q, k, v, scale, doc_ref.global_mask(cu, S, B), out_dtype=q.dtype)
    if ud == 1 and rd == 4:
        assert not doc_blocks.ring_visible(docs, rows, 3, 1) and doc_blocks.ring_visible(docs, rows, 2, 1)
    if ud > 1:                                               # the ring's shard is S / rd rows: entry 1 sees nothing in (rank 1, step 1)
        assert doc_blocks.ring_visible(docs, S // rd, 1, 1)
        assert doc_blocks.block_arrays(docs[0], S // rd, S // rd, 0, S // rd) is not None
        assert doc_blocks.block_arrays(docs[1], S // rd, S // rd, 0, S // rd) is None
    for r in range(ws):
        sl = slice(r * rows, (r + 1) * rows)
        for got, want, tol, name in ((res[r][0], ref[0], TOL["bfloat16"]["out"], "out"), (res[r][1], ref[2], grad_tol("bfloat16", 2), "dq"),
                                     (res[r][2], ref[3], grad_tol("bfloat16", 2), "dk"), (res[r][3], ref[4], grad_tol("bfloat16", 2), "dv")):
            assert_close(got, want[:, sl], *tol, f"ring {rd} rank {r} {name}")


# ---- 8. eight equal documents in one sequence = a batch of eight plain causal launches ---------------------------------------------
def test_documents_equal_a_batch(dev):
    from yunchang_amd import _C
    D, n, L = 64, 8, 128
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(1, n * L, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (4, 2, 2))
    cu = [i * L for i in range(n + 1)]
    rl, kh, _ = _arrays(dev, cu, 0, n * L, 0, n * L)
    out, lse, _ = _fwd(q, k, v, D ** -0.5, True, (rl, kh))
    bq, bk, bv = (t.view(n, L, t.shape[2], D) for t in (q, k, v))
    bout, blse, _ = _fwd(bq, bk, bv, D ** -0.5, True, None, family="wave32")
    want = bout.reshape(1, n * L, 4, D).float()
    # one 16-bit rounding of the plain result: an ulp of bf16 is at most 2^-7 of the value
    assert_close(out.float(), want, 2.0 ** -14, 2.0 ** -7, "out against the batch")
    assert_close(lse, blse.permute(1, 0, 2).reshape(1, 4, n * L), 2e-3, 1e-4, "lse against the batch")     # (fp32: this file's lse bound)
