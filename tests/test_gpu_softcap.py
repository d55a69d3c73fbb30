"""Logit soft-capping on the MI355X: the softcap kernels (flash_fwd_softcap_kernel, flash_bwd_softcap_kernel,
flash_bwd_dkdv_softcap_kernel) against the fp64 reference of tests/test_softcap_cpu.py, through the C ABI, the packed
mode, the ring functions and the USP layer.

Tolerances are golden_util.TOL / grad_tol unwidened.  Every case uses q x 4 and a cap of a few units, so that the capped
reference differs from the uncapped one by more than 10x the tolerance (assert_cap_bites); one case uses the realistic
cap 30 on top."""
import os

import numpy as np
import pytest
import torch

from golden_util import TOL, assert_close, grad_tol
from test_softcap_cpu import assert_cap_bites, make_case, np64, ref_bwd, ref_fwd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import yunchang_amd  # noqa: F401  (loads libusp_hip.so)
    return torch.device("cuda:0")


def _dt(dtype):
    return "bfloat16" if dtype == torch.bfloat16 else "float16"


def _block(dev, q, k, v, do, scale, cap, causal, window=None, k_splits=0, splits=(0, 0), dkdv_heads=0, family=None):
    """One forward + backward through _C at block level -> (out, dq, dk, dv) as fp64 numpy, and the launch kinds."""
    from yunchang_amd import _C
    q, k, v, do = (t.to(dev) for t in (q, k, v, do))
    B, Sq, Hq, D = q.shape
    out = torch.empty_like(q)
    lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=dev)
    _C.flash_fwd(q, k, v, scale, causal, lse, out, k_splits=k_splits, window=window, family=family, softcap=cap)
    kinds = set(_C.last_launch_kinds())
    delta = torch.empty_like(lse)
    _C.bwd_delta(do, out, delta)
    dq, dk, dv = (torch.empty(t.shape, dtype=torch.float32, device=dev) for t in (q, k, v))
    _C.flash_bwd(do, q, k, v, lse, delta, dq, dk, dv, scale, causal, splits=splits, window=window, family=family,
                 dkdv_heads=dkdv_heads, softcap=cap)
    kinds |= set(_C.last_launch_kinds())
    return [np64(t) for t in (out, dq, dk, dv)], kinds


def _check(got, q, k, v, do, scale, cap, causal, window, dtype, what):
    dt = _dt(dtype)
    qn, kn, vn, don = (np64(t) for t in (q, k, v, do))
    ro, _ = ref_fwd(qn, kn, vn, scale, cap, causal, window)
    rg = ref_bwd(don, qn, kn, vn, scale, cap, causal, window)
    assert_close(got[0], ro, *TOL[dt]["out"], f"{what} out")
    for g, r, nm in zip(got[1:], rg, ("dq", "dk", "dv")):
        assert_close(g, r, *grad_tol(dt), f"{what} {nm}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("causal", [True, False])
def test_block_softcap_matches_reference(dev, D, dtype, causal):
    """GQA 8/2, ragged Sq != Sk (bottom-right causal), two batches: forward and both backward launches."""
    q, k, v, do = make_case(2, 200, 328, 8, 2, D, dtype, seed=D + causal)
    scale, cap = D ** -0.5, 3.0
    assert_cap_bites(*(np64(t) for t in (q, k, v, do)), scale, cap, causal, None, TOL[_dt(dtype)]["out"][0],
                     grad_tol(_dt(dtype))[0])
    got, kinds = _block(dev, q, k, v, do, scale, cap, causal)
    _check(got, q, k, v, do, scale, cap, causal, None, dtype, f"D{D} {dtype} causal={causal}")
    assert not any(k_.endswith("row64") for k_ in kinds), kinds


@pytest.mark.parametrize("case", ["window", "k_splits", "cuts_heads1", "cuts_headsG", "cap30"])
def test_block_softcap_composes(dev, case):
    """Softcap with a sliding window, the forward K split, the backward dQ / dK-dV cuts with dkdv_heads 1 and G, and the
    realistic cap 30 (Gemma-2 style) at D = 128."""
    D, G = 128, 4
    q, k, v, do = make_case(1, 384, 384, 8, 8 // G, D, seed=11)
    scale, cap, causal, window = D ** -0.5, 2.0, True, None
    kw = {}
    if case == "window":
        causal, window = False, (96, 40)
    elif case == "k_splits":
        kw = dict(k_splits=3)
    elif case == "cuts_heads1":
        kw = dict(splits=(2, 3), dkdv_heads=1)
    elif case == "cuts_headsG":
        kw = dict(splits=(3, 2), dkdv_heads=G)
    else:
        # q x 4 and k x 4 (exact in bf16): scores of std ~16 reach ~70, so the realistic cap 30 bites.  (q x 16 alone
        # bites too, but its |Q| ~ 64 makes dK's 16-bit rounding error -- 0.15 measured -- exceed the tolerance with or
        # without softcap; spreading the scale over q and k keeps every operand at the magnitude of the other cases.)
        q, k, v, do = make_case(1, 384, 384, 8, 2, D, seed=12)
        k = (k.float() * 4).to(k.dtype)
        cap = 30.0
    assert_cap_bites(*(np64(t) for t in (q, k, v, do)), scale, cap, causal, window, 2e-2, 5e-2)
    got, kinds = _block(dev, q, k, v, do, scale, cap, causal, window=window, **kw)
    _check(got, q, k, v, do, scale, cap, causal, window, torch.bfloat16, case)
    if case == "k_splits":
        assert "fwd_split_merge" in kinds, kinds
    if case.startswith("cuts"):
        assert "reduce_cuts" in kinds and "reduce_heads" in kinds, kinds


def test_block_softcap_merge_in_and_partial_final_rows(dev):
    """Two key halves through the fused LSE merge: the first call leaves fp32 partials, the second merges and finalises
    rows [64, 200) to 16 bits and leaves the others in the fp32 accumulator."""
    from yunchang_amd import _C
    D, cap = 64, 2.5
    q, k, v, do = make_case(1, 256, 320, 4, 2, D, seed=21)
    scale = D ** -0.5
    qd, kd, vd = (t.to(dev) for t in (q, k, v))
    out = torch.zeros_like(qd)
    acc = torch.zeros(qd.shape, dtype=torch.float32, device=dev)
    lse = torch.empty((1, 4, 256), dtype=torch.float32, device=dev)
    _C.flash_fwd(qd, kd[:, :160], vd[:, :160], scale, False, lse, None, acc, False, 0, 0, softcap=cap)
    _C.flash_fwd(qd, kd[:, 160:], vd[:, 160:], scale, False, lse, out, acc, True, 64, 200, softcap=cap)
    ro, rl = ref_fwd(np64(q), np64(k), np64(v), scale, cap, False)
    assert_close(np64(out)[:, 64:200], ro[:, 64:200], *TOL["bfloat16"]["out"], "final rows")
    assert_close(np64(acc)[:, :64], ro[:, :64], 2e-3, 2e-3, "accumulated rows (front)")
    assert_close(np64(acc)[:, 200:], ro[:, 200:], 2e-3, 2e-3, "accumulated rows (back)")
    assert_close(np64(lse), rl, 2e-3, 1e-4, "lse")


@pytest.mark.parametrize("D", [64, 128])
def test_softcap_off_is_bit_identical(dev, D):
    """softcap None / 0 / 0.0 runs exactly the kernels it ran before, with the same results bit for bit."""
    from yunchang_amd import _C
    q, k, v, do = make_case(1, 512, 512, 8, 2, D, seed=5)
    res = []
    for cap in ("absent", None, 0, 0.0):
        kw = {} if cap == "absent" else {"softcap": cap}
        qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
        out = torch.empty_like(qd)
        lse = torch.empty((1, 8, 512), dtype=torch.float32, device=dev)
        _C.flash_fwd(qd, kd, vd, D ** -0.5, True, lse, out, **kw)
        kf = _C.last_launch_kinds()
        delta = torch.empty_like(lse)
        _C.bwd_delta(dod, out, delta)
        dq, dk, dv = (torch.empty(t.shape, dtype=torch.float32, device=dev) for t in (qd, kd, vd))
        _C.flash_bwd(dod, qd, kd, vd, lse, delta, dq, dk, dv, D ** -0.5, True, **kw)
        res.append(((kf, _C.last_launch_kinds()), [t.clone() for t in (out, lse, dq, dk, dv)]))
    for kinds, ts in res[1:]:
        assert kinds == res[0][0]
        assert all(torch.equal(a, b) for a, b in zip(ts, res[0][1]))


def test_unforced_d128_softcap_runs_the_wave32_family(dev):
    """The 64-row kernels decline softcap: an unforced D = 128 call runs the 8 / 4-wave kernels, a forced one fails."""
    q, k, v, do = make_case(1, 2048, 2048, 4, 4, 128, seed=7)
    got, kinds = _block(dev, q, k, v, do, 128 ** -0.5, 4.0, True, k_splits=0)
    assert kinds & {"fwd_wave8", "fwd_wave4"} and {"dkdv_wave8", "dq_wave8"} <= kinds, kinds
    assert not any(x.endswith("row64") for x in kinds), kinds
    with pytest.raises(RuntimeError):
        _block(dev, q, k, v, do, 128 ** -0.5, 4.0, True, family="row64")
    # (without softcap the same call takes 64-row kernels: the decline is the cap's doing)
    _, plain = _block(dev, q, k, v, do, 128 ** -0.5, None, True, k_splits=0)
    assert any(x.endswith("row64") for x in plain), plain


def test_padded_head_dim_softcap_autograd(dev):
    """D = 96 runs on zero-padded copies (kernel_head_dim) with the scale of D = 96; hip_attn_func carries the cap."""
    from yunchang_amd.kernels.attention import hip_attn_func
    D, cap = 96, 3.0
    q, k, v, do = make_case(1, 160, 160, 4, 2, D, seed=9)
    tq, tk, tv = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    out = hip_attn_func(tq, tk, tv, causal=True, softcap=cap)
    out.backward(do.to(dev))
    got = [np64(t) for t in (out, tq.grad, tk.grad, tv.grad)]
    _check(got, q, k, v, do, D ** -0.5, cap, True, None, torch.bfloat16, "D96")


def test_packed_varlen_softcap(dev):
    """Packed mode: three sequences of unequal length through flash_fwd_packed / flash_bwd_packed with softcap."""
    from yunchang_amd import _C
    D, Hq, Hkv, cap = 64, 4, 2, 3.0
    lens = (192, 40, 130)
    T = sum(lens)
    q, k, v, do = (t[0] for t in make_case(1, T, T, Hq, Hkv, D, dtype=torch.float16, seed=13))
    cs = np.concatenate([[0], np.cumsum(lens)])
    tab = torch.tensor([[a, n] for a, n in zip(cs[:-1], lens)], dtype=torch.int32, device=dev)
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    out = torch.empty_like(qd)
    lse = torch.empty((Hq, T), dtype=torch.float32, device=dev)
    _C.flash_fwd_packed(qd, kd, vd, tab, tab, max(lens), max(lens), D ** -0.5, True, lse, out, softcap=cap)
    delta = torch.empty((1, Hq, T), dtype=torch.float32, device=dev)
    _C.bwd_delta(dod[None], out[None], delta)
    dq, dk, dv = (torch.zeros(t.shape, dtype=torch.float32, device=dev) for t in (qd, kd, vd))
    _C.flash_bwd_packed(dod, qd, kd, vd, lse, delta[0], tab, tab, max(lens), max(lens), dq, dk, dv, D ** -0.5, True,
                        softcap=cap)
    for a, n in zip(cs[:-1], lens):
        sl = slice(a, a + n)
        qn, kn, vn, don = (np64(t[sl])[None] for t in (q, k, v, do))
        ro, _ = ref_fwd(qn, kn, vn, D ** -0.5, cap, True)
        rg = ref_bwd(don, qn, kn, vn, D ** -0.5, cap, True)
        assert_close(np64(out[sl])[None], ro, *TOL["float16"]["out"], f"seq {a} out")
        for g, r, nm in zip((dq, dk, dv), rg, ("dq", "dk", "dv")):
            assert_close(np64(g[sl])[None], r, *grad_tol("float16"), f"seq {a} {nm}")


@pytest.fixture(scope="module")
def one_rank(dev):
    import torch.distributed as dist
    import yunchang_amd as Y
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29741")
    own = not dist.is_initialized()
    if own:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    Y.set_seq_parallel_pg(1, 1, 0, 1)
    yield dist
    if own:
        dist.destroy_process_group()


def test_varlen_ring_and_usp_layer_single_rank(dev, one_rank):
    """zigzag_ring_flash_attn_varlen_func and LongContextAttention (default path) at world size 1, forward + backward."""
    import yunchang_amd as Y
    cap, D = 3.0, 128
    lens = (256, 96)
    T = sum(lens)
    q, k, v, do = (t[0] for t in make_case(1, T, T, 4, 2, D, seed=17))
    cs = np.concatenate([[0], np.cumsum(lens)])
    tq, tk, tv = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    cu = torch.tensor(cs, dtype=torch.int32, device=dev)
    out = Y.zigzag_ring_flash_attn_varlen_func(tq, tk, tv, cu, max(lens), causal=True, softcap=cap, group=one_rank.group.WORLD)
    out.backward(do.to(dev))
    for a, n in zip(cs[:-1], lens):
        sl = slice(a, a + n)
        qn, kn, vn, don = (np64(t[sl])[None] for t in (q, k, v, do))
        ro, _ = ref_fwd(qn, kn, vn, D ** -0.5, cap, True)
        rg = ref_bwd(don, qn, kn, vn, D ** -0.5, cap, True)
        assert_close(np64(out[sl])[None], ro, *TOL["bfloat16"]["out"], "varlen out")
        for g, r, nm in zip((tq.grad, tk.grad, tv.grad), rg, ("dq", "dk", "dv")):
            assert_close(np64(g[sl])[None], r, *grad_tol("bfloat16"), f"varlen {nm}")

    q, k, v, do = make_case(2, 256, 256, 8, 2, D, seed=19)
    tq, tk, tv = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    out = Y.LongContextAttention(ring_impl_type="zigzag")(tq, tk, tv, causal=True, softcap=cap)
    out.backward(do.to(dev))
    _check([np64(t) for t in (out, tq.grad, tk.grad, tv.grad)], q, k, v, do, D ** -0.5, cap, True, None, torch.bfloat16,
           "LongContextAttention")


def test_usp_grid_2x2_through_rccl(dev, one_rank, monkeypatch):
    """Ulysses 2 x ring 2 (zigzag, causal, GQA) on a virtual grid of one device, every exchange and ring transfer through
    RCCL: the layer's pipelined path with softcap against the fp64 reference of the global tensors."""
    from oracle import usp_oracle as O
    from virtual_grid import Ctx, VirtualGrid, patch_dist, run_grid
    grid = VirtualGrid(2, 2, one_rank)
    AL = patch_dist(monkeypatch, grid)
    monkeypatch.setattr(AL, "_FILL_ITEMS", 1)
    cap, D, ws = 3.0, 64, 4
    q, k, v, do = make_case(1, 512, 512, 8, 4, D, seed=23)
    shard = lambda x, r: np.ascontiguousarray(O.EXTRACT["zigzag"](x, r, ws, 2, 2))     # the grid's rank layout
    loc = [[torch.from_numpy(shard(t.float().numpy(), r)).to(q.dtype).to(dev) for t in (q, k, v, do)] for r in range(ws)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(ws)]
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        lq, lk, lv, ldo = loc[r]
        upg, rpg = grid.groups_of(r)
        ctx = Ctx()
        with torch.cuda.stream(streams[r]):
            out = AL._AsyncUSPFunc.forward(ctx, lq, lk, lv, None, True, upg, rpg, "zigzag", AL._MAX_GROUPS, cap)
            grads = AL._AsyncUSPFunc.backward(ctx, ldo)[:3]
        return (out,) + tuple(grads)

    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    qn, kn, vn, don = (np64(t) for t in (q, k, v, do))
    ro, _ = ref_fwd(qn, kn, vn, D ** -0.5, cap, True)
    truth = (ro,) + tuple(ref_bwd(don, qn, kn, vn, D ** -0.5, cap, True))
    for r in range(ws):
        for got, want, nm in zip(res[r], truth, ("out", "dq", "dk", "dv")):
            want_r = shard(want, r)
            tol = TOL["bfloat16"]["out"] if nm == "out" else grad_tol("bfloat16")
            assert_close(np64(got), want_r, *tol, f"rank {r} {nm}")
