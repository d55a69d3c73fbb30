"""Head dim 256 on the GPU (run with -m gpu on an MI355X): the kernel family of csrc/usp_flash_fwd_d256.hip and
csrc/usp_flash_bwd_d256.hip through hip_attn_forward / hip_attn_backward / hip_attn_func, against the fp64 oracle
(oracle.usp_oracle.block_fwd / block_bwd) within the project's stated tolerances (golden_util.TOL; lse 2e-3 / 1e-4).  The entry
points serve head dims above 128 after set_head_dim_256(True): on for this module, restored behind it.  The launch-depth, needle,
layout and ring tests drive the C ABI binding (_C.flash_fwd / _C.flash_bwd) and the layer's function as the suite's harnesses do."""
import os

import numpy as np
import pytest
import torch

from golden_util import TOL, assert_close, round_to
from oracle import usp_oracle as O

pytestmark = pytest.mark.gpu
D256_KINDS = {"fwd": ("fwd_d256",), "bwd": ("dkdv_d256", "dq_d256")}


@pytest.fixture(scope="module")
def dev():
    from yunchang_amd import _C
    from yunchang_amd.kernels import set_head_dim_256
    _C.load()
    prev = set_head_dim_256(True)
    yield torch.device("cuda:0")
    set_head_dim_256(prev)


def _t(x, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(getattr(torch, dt)).to(dev)


def _f(t):
    return t.detach().float().cpu().numpy()


def _rand(shape, dt, seed):
    return round_to(np.random.RandomState(seed).standard_normal(shape).astype(np.float32), dt)


SHAPES = [
    # B, Sq, Sk, Hq, Hkv, causal, dtype
    (1, 1, 1, 1, 1, True, "float16"),
    (2, 77, 77, 2, 2, True, "bfloat16"),          # less than one item
    (1, 200, 333, 3, 1, True, "bfloat16"),        # ragged, bottom-right, GQA 3
    (1, 333, 200, 2, 2, True, "float16"),         # rows with no visible key
    (1, 384, 640, 4, 2, False, "bfloat16"),
    (1, 130, 1, 2, 1, False, "bfloat16"),
    (1, 129, 193, 2, 1, True, "bfloat16"),        # one-row second item, one-key fourth tile
]


@pytest.mark.parametrize("B,Sq,Sk,Hq,Hkv,causal,dt", SHAPES)
def test_forward_backward_vs_oracle(dev, B, Sq, Sk, Hq, Hkv, causal, dt):
    from yunchang_amd import _C
    from yunchang_amd.kernels import hip_attn_backward, hip_attn_forward
    D = 256
    q, k, v, do = (_rand(s, dt, i) for i, s in enumerate([(B, Sq, Hq, D), (B, Sk, Hkv, D), (B, Sk, Hkv, D), (B, Sq, Hq, D)]))
    tq, tk, tv, tdo = (_t(x, dt, dev) for x in (q, k, v, do))
    out, lse = hip_attn_forward(tq, tk, tv, 0.0, None, causal=causal)
    assert _C.last_launch_kinds() == D256_KINDS["fwd"]
    ro, rl = O.block_fwd(q, k, v, None, causal)
    assert_close(_f(out), ro, *TOL[dt]["out"], "out")
    lse_h, fin = _f(lse), np.isfinite(rl)
    assert (np.isfinite(lse_h) == fin).all() and (lse_h[~fin] == -np.inf).all(), "empty rows must give lse = -inf"
    assert_close(lse_h[fin], rl[fin], 2e-3, 1e-4, "lse")
    assert (np.abs(_f(out))[~np.broadcast_to(fin.transpose(0, 2, 1)[..., None], ro.shape)] == 0).all()
    o16 = round_to(ro.astype(np.float32), dt)
    dq, dk, dv = (torch.empty_like(t) for t in (tq, tk, tv))
    hip_attn_backward(tdo, tq, tk, tv, _t(o16, dt, dev), torch.from_numpy(rl.astype(np.float32)).to(dev), dq, dk, dv, 0.0, None, causal)
    assert _C.last_launch_kinds() == D256_KINDS["bwd"]
    for got, want, name in zip((dq, dk, dv), O.block_bwd(do, q, k, v, o16, rl, None, causal), ("dq", "dk", "dv")):
        assert_close(_f(got), want, *TOL[dt]["grad"], name)


def test_running_max_jumps(dev):
    """test_gpu_parity.py::test_softmax_rescale_branch's inputs at D = 256: one key per 64-key tile is aligned with row 300, so its
    maximum grows tile after tile."""
    from yunchang_amd.kernels import hip_attn_forward
    dt, (B, S, H, D) = "bfloat16", (1, 512, 1, 256)
    rs = np.random.RandomState(3)
    q = rs.standard_normal((B, S, H, D)).astype(np.float32)
    k = rs.standard_normal((B, S, H, D)).astype(np.float32) * 0.1
    for t in range(S // 64):
        k[0, 64 * t + 5, 0] = q[0, 300, 0] * (0.5 + 0.25 * t)
    v = rs.standard_normal((B, S, H, D)).astype(np.float32)
    q, k, v = (round_to(x, dt) for x in (q, k, v))
    out, lse = hip_attn_forward(_t(q, dt, dev), _t(k, dt, dev), _t(v, dt, dev), causal=False)
    ro, rl = O.block_fwd(q, k, v, None, False)
    assert_close(_f(out), ro, *TOL[dt]["out"], "out")
    assert_close(_f(lse), rl, 2e-3, 1e-4, "lse")


@pytest.mark.parametrize("D", [160, 192])
def test_padded_head_dims_autograd(dev, D):
    """Head dims between 128 and 256 run on zero-padded copies at the scale of the unpadded dim, with no host synchronisation."""
    from yunchang_amd.kernels import hip_attn_func
    dt, (B, S, Hq, Hkv) = "bfloat16", (1, 200, 2, 1)
    q, k, v, do = (_rand(s, dt, 40 + i) for i, s in enumerate([(B, S, Hq, D), (B, S, Hkv, D), (B, S, Hkv, D), (B, S, Hq, D)]))
    tq, tk, tv = (_t(x, dt, dev).requires_grad_(True) for x in (q, k, v))
    tdo = _t(do, dt, dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = hip_attn_func(tq, tk, tv, causal=True)
        out.backward(tdo)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ro, rl = O.block_fwd(q, k, v, None, True)                 # (default scale: D ** -0.5 of the unpadded dim)
    assert_close(_f(out), ro, *TOL[dt]["out"], "out")
    for got, want, name in zip((tq.grad, tk.grad, tv.grad), O.block_bwd(do, q, k, v, ro, rl, None, True), ("dq", "dk", "dv")):
        assert_close(_f(got), want, *TOL[dt]["grad"], name)


def _verdicts(what, got, want, dt, Sq, Sk, G):
    """The suite's comparator (needle_inputs.verdicts: golden_util.TOL, lse 2e-3 / 1e-4, long_sum_atol on sums of >= 1000 products)."""
    import needle_inputs as NI
    ver = NI.verdicts(got, want, dt, Sq, Sk, G)
    print(f"[d256] {what}: " + " ".join(f"{n}={r:.3f}" for n, (_, r) in ver.items()))
    bad = {n: round(r, 3) for n, (ok, r) in ver.items() if not ok}
    assert not bad, f"{what}: out of tolerance, worst error / bound {bad}"


def _c_abi_fwd_bwd(dev, q, k, v, do, dt, causal, ro, rl, **kw):
    """One forward and one backward launch on the C ABI (lse from the oracle, `out` the oracle's rounded to 16 bits)."""
    from yunchang_amd import _C
    tq, tk, tv, tdo = (_t(x, dt, dev) for x in (q, k, v, do))
    scale = q.shape[-1] ** -0.5
    out = torch.empty_like(tq)
    lse = torch.empty(q.shape[0], q.shape[2], q.shape[1], dtype=torch.float32, device=dev)
    _C.flash_fwd(tq, tk, tv, scale, causal, lse, out=out, **kw)
    assert _C.last_launch_kinds() == D256_KINDS["fwd"]
    delta = torch.empty_like(lse)
    _C.bwd_delta(tdo, _t(round_to(ro.astype(np.float32), dt), dt, dev), delta)
    dq, dk, dv = (torch.empty_like(t) for t in (tq, tk, tv))
    _C.flash_bwd(tdo, tq, tk, tv, torch.from_numpy(np.ascontiguousarray(rl, dtype=np.float32)).to(dev), delta, None, None, None, scale, causal,
                 dq16=dq, dk16=dk, dv16=dv, **kw)
    assert _C.last_launch_kinds() == D256_KINDS["bwd"]
    torch.cuda.synchronize()
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)


def test_multi_pass_launch_every_element(dev):
    """More items than resident workgroups: 2 x 8 x 17 = 272 forward and dQ items on 256 CUs (the second pass of ItemWalk: LDS
    buffers, accumulators and row statistics reused by a second item), 68 dK/dV items looping 4 query heads.  Every element against
    the oracle, computed in row chunks (a causal chunk of rows [a, b) sees keys [0, b): the bottom-right alignment), and the
    persistent launch bit for bit against USP_LAUNCH_INTERLEAVE (one workgroup per item)."""
    dt, (B, S, Hq, Hkv, D), step = "bfloat16", (2, 2176, 8, 2, 256), 544
    q, k, v, do = (_rand(s, dt, 20 + i) for i, s in enumerate([(B, S, Hq, D), (B, S, Hkv, D), (B, S, Hkv, D), (B, S, Hq, D)]))
    ro, rl = np.empty((B, S, Hq, D)), np.empty((B, Hq, S))
    for a in range(0, S, step):
        ro[:, a:a + step], rl[:, :, a:a + step] = O.block_fwd(q[:, a:a + step], k[:, :a + step], v[:, :a + step], None, True)
    o16 = round_to(ro.astype(np.float32), dt)
    want = dict(out=ro, lse=rl, dq=np.empty_like(ro), dk=np.zeros((B, S, Hkv, D)), dv=np.zeros((B, S, Hkv, D)))
    for a in range(0, S, step):
        g = O.block_bwd(do[:, a:a + step], q[:, a:a + step], k[:, :a + step], v[:, :a + step], o16[:, a:a + step], rl[:, :, a:a + step], None, True)
        want["dq"][:, a:a + step] = g[0]
        want["dk"][:, :a + step] += g[1]
        want["dv"][:, :a + step] += g[2]
    got = _c_abi_fwd_bwd(dev, q, k, v, do, dt, True, ro, rl)
    one = _c_abi_fwd_bwd(dev, q, k, v, do, dt, True, ro, rl, interleave=True)
    for n in got:
        assert torch.equal(got[n].view(torch.int16 if n != "lse" else torch.int32), one[n].view(torch.int16 if n != "lse" else torch.int32)), \
            f"{n}: the persistent launch differs from one workgroup per item"
    _verdicts("multi-pass", {n: _f(t) for n, t in got.items()}, want, dt, S, S, Hq // Hkv)


def test_needle_inputs(dev):
    """tests/needle_inputs.py at D = 256: the softmax mass of every row sits on one needle key per 64-key tile, so a lost, doubled or
    mispaired key tile (or a wrong head of the KV group) is an O(1) error in out and in all three gradients."""
    import needle_inputs as NI
    dt, (S, Hq, Hkv, D) = "bfloat16", (1000, 4, 2, 256)
    edges = NI.mask_edges(NI.sample_rows(S, 10), S, S, causal=True) + NI.key_block_edges(S, S, True, every=2, per=2)
    nd = NI.make(S, S, Hq, Hkv, D, dt, 3, seed=11, edges=edges)
    NI.assert_needle_conditions(nd, NI.sample_rows(S, 10), D ** -0.5, lambda r: np.arange(S) <= r, "d256")
    ro, rl = O.block_fwd(nd.q, nd.k, nd.v, None, True)
    want = dict(zip(("dq", "dk", "dv"), O.block_bwd(nd.do, nd.q, nd.k, nd.v, round_to(ro.astype(np.float32), dt), rl, None, True)), out=ro, lse=rl)
    got = _c_abi_fwd_bwd(dev, nd.q, nd.k, nd.v, nd.do, dt, True, ro, rl)
    _verdicts("needle", {n: _f(t) for n, t in got.items()}, want, dt, S, S, Hq // Hkv)


LAYOUTS = [
    # call, seed (walks the layout kinds), extra arguments of layout_util.Case
    ("fwd", 3, dict()),
    ("fwd", 6, dict(ring=(141, 64, 160))),                  # two calls: acc only, then merge_in with rows 64..159 final
    ("bwd", 2, dict(forms=("f32+", "h16", "h16+"))),
    ("bwd", 5, dict(forms=("h16", "f32", "f32+"))),
]


@pytest.mark.parametrize("call,seed,kw", LAYOUTS, ids=lambda v: str(v).replace(" ", ""))
def test_strided_layouts_in_poisoned_memory(dev, call, seed, kw):
    """The ragged GQA case with every tensor a strided view of its own inside sentinel-filled memory (tests/layout_util.py): bit for
    bit the contiguous run, that run within TOL of the oracle, nothing written outside the views, untouched rows untouched."""
    import layout_util as LU
    from test_gpu_layouts import HipOps
    kinds = set(D256_KINDS[call])
    case = LU.Case(1, 200, 333, 3, 1, 256, True, "bfloat16", kinds=kinds, **kw)
    got = (LU.check_fwd_case if call == "fwd" else LU.check_bwd_case)(HipOps(), case, seed, dev)
    assert all(set(g) == kinds for g in (got if call == "fwd" else [got]))


@pytest.fixture(scope="module")
def nccl_single():
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29747")
    own = not dist.is_initialized()
    if own:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    yield dist
    if own:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("ud,rd,impl", [(1, 2, "basic"), (1, 2, "zigzag"), (2, 1, "basic"), (2, 2, "zigzag")])
def test_rings_and_layer_on_the_virtual_grid(dev, nccl_single, monkeypatch, ud, rd, impl):
    """The fused merge and the final ranges of the forward epilogue, accum_dq / accum_dk / accum_dv and USP_LAUNCH_INTERLEAVE, as the
    schedules use them: the layer's function (what LongContextAttention.forward runs: Ulysses exchange, ring, exchange back) on a
    virtual ud x rd grid with S_local = 192 -- the basic and the zigzag ring at degree 2, Ulysses at degree 2, the 2 x 2 grid --
    forward and backward against the single-device fp64 result."""
    from golden_util import grad_tol
    from virtual_grid import Ctx, VirtualGrid, patch_dist, run_grid
    dt, (Hq, Hkv, D), ws = "bfloat16", (4, 2, 256), ud * rd
    S = 192 * ws
    q, k, v, do = (_rand(s, dt, 60 + i) for i, s in enumerate([(1, S, Hq, D), (1, S, Hkv, D), (1, S, Hkv, D), (1, S, Hq, D)]))
    grid = VirtualGrid(ud, rd, nccl_single)
    AL = patch_dist(monkeypatch, grid)
    monkeypatch.setattr(AL, "_FILL_ITEMS", 1)
    import yunchang_amd.comm.relay_exchange as RX
    monkeypatch.setitem(RX._OVERRIDE, "relay", False)
    shard = lambda x, r: O.EXTRACT[impl](x, r, ws, rd, ud)
    loc = [[_t(shard(x, r), dt, dev) for x in (q, k, v, do)] for r in range(ws)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(ws)]
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        upg, rpg = grid.groups_of(r)
        ctx = Ctx()
        with torch.cuda.stream(streams[r]):
            out = AL._AsyncUSPFunc.forward(ctx, *loc[r][:3], None, True, upg, rpg, impl, AL._MAX_GROUPS)
            return (out,) + tuple(AL._AsyncUSPFunc.backward(ctx, loc[r][3])[:3])

    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    ro, rl = O.block_fwd(q, k, v, None, True)
    want = (ro,) + tuple(O.block_bwd(do, q, k, v, ro, rl, None, True))
    for r in range(ws):
        for got, w, name in zip(res[r], want, ("out", "dq", "dk", "dv")):
            tol = TOL[dt]["out"] if name == "out" else grad_tol(dt, Hq // Hkv)
            assert_close(_f(got), shard(w, r), *tol, f"{ud}x{rd} {impl} rank {r} {name}")
