"""A sliding window over GLOBAL positions on the basic ring (ring degree > 1, USP_RING_WINDOW=global), CPU side:
the block planner (ring/window_blocks.py) against the brute-force global mask, the diagonal shift of the C ABI (USP_ATTN_SHIFT)
at the host API, and the ring forward / backward on gloo with an oracle-style block backend that takes `shift`, against exact
attention on the unsharded tensors (tests/shift_ref.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import shift_ref
from dist_util import run_distributed
from golden_util import TOL, assert_close, grad_tol
from oracle_backend import OracleBlockBackend, _operand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference of these tests against the project's fp64 reference -------------------------------------------------------
@pytest.mark.parametrize("Sq,Sk,Hq,Hkv,causal,window,softcap", [(24, 40, 4, 2, True, None, None), (32, 32, 2, 2, False, (5, 3), None),
                                                                (40, 24, 4, 1, True, (7, -1), None), (33, 20, 2, 2, False, (3, -1), 2.5)])
def test_shift_ref_is_attn_ref_at_shift_zero(Sq, Sk, Hq, Hkv, causal, window, softcap):
    import attn_ref_torch as A
    g = torch.Generator().manual_seed(5)
    q, k, v, do = (torch.randn(2, s, h, 16, generator=g, dtype=torch.float64) for s, h in ((Sq, Hq), (Sk, Hkv), (Sk, Hkv), (Sq, Hq)))
    scale = 0.25
    o, l = shift_ref.ref_fwd(q, k, v, scale, causal, window, 0, softcap)
    o2, l2 = A.ref_fwd(q, k, v, scale, causal, window, softcap)
    assert_close(o, o2, 1e-12, 1e-12, "out")
    assert_close(l, l2, 1e-12, 1e-12, "lse")
    o16 = o.to(torch.bfloat16)
    got = shift_ref.ref_bwd(do, q, k, v, o16, l, scale, causal, window, 0, softcap)
    want = A.ref_bwd(do, q, k, v, o16, l2, scale, causal, window, softcap)[:3]
    for a, b, name in zip(got, want, ("dq", "dk", "dv")):
        assert_close(a, b, 1e-11, 1e-11, name)


def test_shift_ref_shift_is_a_moved_diagonal():
    """visible(shift) is the (Sq, Sk) window of a larger mask: the definition, stated independently."""
    big = shift_ref.visible(96, 96, True, (20, 0), 0)
    assert torch.equal(shift_ref.visible(32, 32, True, (20, 0), 32), big[64:96, 32:64])
    assert torch.equal(shift_ref.visible(32, 32, False, (20, 7), -32), shift_ref.visible(96, 96, False, (20, 7), 0)[0:32, 32:64])


# ---- 1. the planner against brute force ---------------------------------------------------------------------------------------------
def _global_mask(S, causal, wl, wr):
    i, j = np.arange(S)[:, None], np.arange(S)[None, :]
    m = np.ones((S, S), bool)
    if wl >= 0:
        m &= j >= i - wl
    if wr >= 0:
        m &= j <= i + wr
    if causal:
        m &= j <= i
    return m


def _launch_mask(c, blk):
    """The mask the kernels apply for a launch description (include/usp_hip.h: USP_ATTN_WINDOW + USP_ATTN_SHIFT), Sq = Sk = c."""
    wl, wr = blk.window if blk.window is not None else (-1, -1)
    if blk.causal:
        wr = 0
    off = blk.shift or 0
    i, j = np.arange(c)[:, None] + off, np.arange(c)[None, :]
    m = np.ones((c, c), bool)
    if wl >= 0:
        m &= j >= i - wl
    if wr >= 0:
        m &= j <= i + wr
    return m


def _span(any_true):
    idx = np.flatnonzero(any_true)
    return (int(idx[0]), int(idx[-1]) + 1)


def test_planner_against_the_brute_force_global_mask():
    from yunchang_amd.ring import window_blocks as W
    n_blocks = n_empty = n_full = 0
    for P in range(1, 6):
        for c in (1, 3, 8):
            S = P * c
            for wl in (-1, 0, 1, c - 1, c, c + 1, 2 * c, 3 * c + 1, S):
                for wr in (-1, 0, 1, c, 2 * c + 1):
                    for causal in (False, True):
                        if wl < 0 and wr < 0 and not causal:
                            continue                                   # no bound at all: not a window
                        G = _global_mask(S, causal, wl, wr)
                        union = np.zeros_like(G)
                        for r in range(P):
                            assert 0 in W.compute_steps(P, c, causal, wl, wr, r), "step 0 is never empty"
                            for s in range(P):
                                src = (r - s) % P
                                sub = G[r * c:(r + 1) * c, src * c:(src + 1) * c]
                                blk = W.plan_block(P, c, causal, wl, wr, r, s)
                                what = (P, c, wl, wr, causal, r, s)
                                n_blocks += 1
                                if not sub.any():
                                    assert blk is None, what
                                    n_empty += 1
                                    continue
                                assert blk is not None, what
                                m = _launch_mask(c, blk)
                                assert np.array_equal(m, sub), what
                                union[r * c:(r + 1) * c, src * c:(src + 1) * c] = m
                                assert blk.full == bool(sub.all()), what
                                n_full += blk.full
                                assert blk.keys == _span(sub.any(0)) and blk.rows == _span(sub.any(1)), what
                                # normalised: a bound is in the launch exactly when it cuts something, the right bound 0 is `causal`
                                right = 0 if causal else wr
                                shift = (r - src) * c
                                i, j = np.arange(c)[:, None] + shift, np.arange(c)[None, :]
                                left_bites = wl >= 0 and bool((j < i - wl).any())
                                right_bites = right >= 0 and bool((j > i + right).any())
                                assert (blk.window is not None and blk.window[0] >= 0) == left_bites, what
                                has_r = blk.causal or (blk.window is not None and blk.window[1] >= 0)
                                assert has_r == right_bites and blk.causal == (right_bites and right == 0), what
                                assert (blk.shift is None) == (blk.full or shift == 0), what
                        assert np.array_equal(union, G), (P, c, wl, wr, causal)
                        # both ends of every K/V transfer agree
                        for a in range(P):
                            for s in range(1, P):
                                b = (a + s) % P
                                sends = s in W.send_steps(P, c, causal, wl, wr, a)
                                assert sends == (s in W.recv_steps(P, c, causal, wl, wr, b)), (P, c, wl, wr, causal, a, s)
                                assert sends == bool(G[b * c:(b + 1) * c, a * c:(a + 1) * c].any())
    assert n_blocks == 14685 and 0 < n_empty < n_blocks and n_full > 0, (n_blocks, n_empty, n_full)


def test_plan_object_and_launch_keywords():
    from yunchang_amd.ring.window_blocks import WindowPlan, plan_block
    plan = WindowPlan(4, 64, True, 100, 0, 3)
    assert plan.steps == [0, 1, 2] and plan.recv == [1, 2] and plan.send == []
    assert WindowPlan(4, 64, True, 100, 0, 0).send == [1, 2] and WindowPlan(4, 64, True, 100, 0, 0).steps == [0]
    b0, b1, b2 = (plan.block(s) for s in plan.steps)
    assert (b0.causal, b0.window, b0.shift) == (True, None, None) and b0.launch_kw() == {}      # 63 - 100 < 0: the left bound is dropped
    assert (b1.causal, b1.window, b1.shift) == (False, (100, -1), 64) and b1.launch_kw() == {"window": (100, -1), "shift": 64}
    assert b2.keys == (28, 64) and b2.rows == (0, 36) and plan.key_extent(3, 2) == slice(28, 64)
    assert plan.block(3) is None and plan.key_extent(3, 3) is None
    full = plan_block(3, 8, False, -1, 20, 2, 1)                       # (-1, 20) towards an earlier chunk: nothing bites
    assert full.full and full.launch_kw() == {} and full.keys == (0, 8)
    with pytest.raises(ValueError):
        WindowPlan(2, 1 << 29, True, 4, 0, 0)


# ---- 2. the C ABI at the host: what is refused before any launch -------------------------------------------------------------------
def _lib():
    from yunchang_amd import _C
    if not os.path.exists(_C.lib_path()):
        pytest.fail("libusp_hip.so is not built: run __graft_entry__.build() first")
    return _C, _C.load()


def _args(_C, cls, addr):
    a = cls()
    a.dtype, a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D = 0, 1, 16, 16, 2, 2, 128
    a.softmax_scale = 0.125
    a.lse = addr
    if cls is _C.UspBwdArgs:
        a.delta = addr
        a.dout.ptr = addr
    a.q.ptr = a.k.ptr = a.v.ptr = addr
    outs = (a.dq, a.dk, a.dv) if cls is _C.UspBwdArgs else (a.out,)
    if cls is _C.UspFwdArgs:
        a.final_end = a.Sq
    for t in outs:
        t.ptr = addr
    for t in (a.q, a.k, a.v) + outs + ((a.dout,) if cls is _C.UspBwdArgs else ()):
        t.stride_b, t.stride_s, t.stride_h = 16 * 2 * 128, 2 * 128, 128
    return a


def test_abi_shift_flag_and_field():
    import re
    _C, L = _lib()
    txt = open(os.path.join(ROOT, "include", "usp_hip.h")).read()
    assert _C.USP_ATTN_SHIFT == 128 == int(re.search(r"#define USP_ATTN_SHIFT (\d+)", txt).group(1))
    assert L.usp_attn_features() & _C.USP_ATTN_SHIFT
    assert L.usp_attn_features() & _C.USP_ATTN_WINDOW and L.usp_attn_features() & _C.USP_ATTN_SOFTCAP
    assert L.usp_abi_version() == 7
    # the field sits in what was padding in front of the first tensor: nothing else moved, nothing grew
    for cls, first in ((_C.UspFwdArgs, "q"), (_C.UspBwdArgs, "dout")):
        assert getattr(cls, "mask_shift").offset == 36 and getattr(cls, "softmax_scale").offset == 32
        assert getattr(cls, first).offset == 40
        assert cls._fields_[-1] == ("softcap", ctypes.c_float)
        no_field = type("Old", (ctypes.Structure,), {"_fields_": [f for f in cls._fields_ if f[0] != "mask_shift"]})
        assert ctypes.sizeof(no_field) == ctypes.sizeof(cls)
        assert all(getattr(no_field, n).offset == getattr(cls, n).offset for n, _ in no_field._fields_)


def test_abi_rejects_bad_shift_without_launch():
    """Host memory stands in for the device pointers: every call below must return before anything is launched."""
    _C, L = _lib()
    buf = ctypes.create_string_buffer(1 << 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    seq = (ctypes.c_int32 * 2)(0, 16)
    for cls, call in ((_C.UspFwdArgs, L.usp_flash_fwd), (_C.UspBwdArgs, L.usp_flash_bwd)):
        for bad in (1 << 30, -(1 << 30), (1 << 31) - 1):
            a = _args(_C, cls, addr)
            a.causal, a.flags, a.mask_shift = 1, _C.USP_ATTN_SHIFT, bad
            assert call(ctypes.byref(a), None) == -1, bad
        a = _args(_C, cls, addr)                       # without the bit the field is not read: the call gets as far as the
        a.flags, a.mask_shift = _C.USP_ATTN_WINDOW, 1 << 30        # refusal of a packed batch with a window
        a.window_left, a.window_right = 4, -1
        a.seq_q = a.seq_k = ctypes.addressof(seq)
        if cls is _C.UspBwdArgs:
            a.total_k = 16
        assert call(ctypes.byref(a), None) == -2
        a.flags |= _C.USP_ATTN_SHIFT                    # ... and with it the range check comes first
        assert call(ctypes.byref(a), None) == -1
        a = _args(_C, cls, addr)                       # a packed batch with the bit
        a.causal, a.flags, a.mask_shift = 1, _C.USP_ATTN_SHIFT, 16
        a.seq_q = a.seq_k = ctypes.addressof(seq)
        if cls is _C.UspBwdArgs:
            a.total_k = 16
        assert call(ctypes.byref(a), None) == -2
        a = _args(_C, cls, addr)                       # the 64-row family forced, with a left bound
        a.flags, a.mask_shift = _C.USP_ATTN_SHIFT | _C.USP_ATTN_WINDOW | _C.USP_FORCE_ROW64, 16
        a.window_left, a.window_right = 4, -1
        assert call(ctypes.byref(a), None) == -2
        a.softmax_scale = 0.0                          # the existing checks still come first
        assert call(ctypes.byref(a), None) == -1


def test_binding_refuses_a_shift_out_of_range_and_a_library_without_the_bit(monkeypatch):
    from yunchang_amd import _C
    with pytest.raises(ValueError):
        _C._shift(1 << 30)
    assert _C._shift(None) is None and _C._shift(0) == 0 and _C._shift(-5) == -5

    class Old:
        @staticmethod
        def usp_attn_features():
            return _C.USP_ATTN_WINDOW | _C.USP_ATTN_SOFTCAP
    monkeypatch.setattr(_C, "load", lambda: Old)
    with pytest.raises(RuntimeError):
        _C._set_shift(_C.UspFwdArgs(), 3)
    a = _C.UspFwdArgs()
    _C._set_shift(a, None)
    assert a.flags == 0


# ---- 3. the ring on gloo ------------------------------------------------------------------------------------------------------------------
class ShiftOracleBackend(OracleBlockBackend):
    """The oracle backend with the block launches restated in torch fp64 (tests/shift_ref.py) so that they take `shift`; operand
    constraints asserted as oracle_backend does.  Logs ("fwd" | "bwd", causal, window, shift, merge_in, final_begin, final_end)."""

    def __init__(self):
        super().__init__()
        self.launches = []

    def fwd(self, q, k, v, softmax_scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None,
            window=None, k_splits=None, shift=None, softcap=None):
        Sq = q.shape[1]
        fe = Sq if final_end is None else final_end
        for t, what in ((q, "q"), (k, "k"), (v, "v"), (acc, "acc")):
            _operand(t, what)
        _operand(out, "out", 8, 8)
        assert lse.stride(-1) == 1 and lse.dtype == torch.float32 and tuple(lse.shape) == (q.shape[0], q.shape[2], Sq)
        assert (fe <= final_begin or out is not None) and ((final_begin <= 0 and fe >= Sq) or acc is not None) \
            and (not merge_in or acc is not None), "final rows need `out`, the others (and a merge) need `acc`"
        assert shift is None or abs(shift) < 1 << 30
        self.launches.append(("fwd", bool(causal), window, shift, bool(merge_in), final_begin, fe))
        bo, bl = shift_ref.ref_fwd(q, k, v, softmax_scale, causal, window, shift or 0, softcap)
        if merge_in:
            old_l = lse.to(torch.float64)
            new_l = torch.logaddexp(old_l, bl)
            fin = torch.isfinite(new_l)
            safe = torch.where(fin, new_l, torch.zeros_like(new_l))
            w_old = torch.where(fin, torch.exp(old_l - safe), torch.zeros_like(safe)).transpose(1, 2)[..., None]
            w_blk = torch.where(fin, torch.exp(bl - safe), torch.zeros_like(safe)).transpose(1, 2)[..., None]
            bo, bl = acc.to(torch.float64) * w_old + bo * w_blk, new_l
        lse.copy_(bl)
        if fe > final_begin:
            out[:, final_begin:fe].copy_(bo[:, final_begin:fe])
        if final_begin > 0:
            acc[:, :final_begin].copy_(bo[:, :final_begin])
        if fe < Sq:
            acc[:, fe:].copy_(bo[:, fe:])

    def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale, causal, accum_dq=False, accum_dk=False, accum_dv=False,
            dq16=None, dk16=None, dv16=None, window=None, only=None, shift=None, softcap=None):
        assert only is None
        for t, what in ((dout, "dout"), (q, "q"), (k, "k"), (v, "v"), (dq, "dq"), (dk, "dk"), (dv, "dv")):
            _operand(t, what)
        for t, what in ((dq16, "dq16"), (dk16, "dk16"), (dv16, "dv16")):
            _operand(t, what, 8, 8)
        assert lse.dtype == torch.float32 and delta.dtype == torch.float32 and lse.shape == delta.shape
        self.launches.append(("bwd", bool(causal), window, shift, bool(accum_dq)))
        # (the block contract takes delta, not out: an `out` with rowsum(dout * out) = delta is dout * delta / |dout|^2)
        do64 = dout.to(torch.float64)
        fake_out = do64 * (delta.to(torch.float64).transpose(1, 2) / do64.square().sum(-1).clamp_min(1e-300))[..., None]
        grads = shift_ref.ref_bwd(dout, q, k, v, fake_out, lse, softmax_scale, causal, window, shift or 0, softcap)
        for g, dst, d16, accum in zip(grads, (dq, dk, dv), (dq16, dk16, dv16), (accum_dq, accum_dk, accum_dv)):
            tot = g + dst.to(torch.float64) if accum else g
            (d16 if d16 is not None else dst).copy_(tot)


CASES = [((40, 0), True), ((100, 0), True), ((0, 0), True), ((30, 20), False), ((-1, 10), False)]
B, HQ, HKV, D = 2, 4, 2, 32


def _inputs(ws):
    g = torch.Generator().manual_seed(7)
    return [torch.randn(B, 64 * ws, h, D, generator=g).to(torch.bfloat16) for h in (HQ, HKV, HKV, HQ)]


def _ring_worker(rank, ws, ud, rd):
    import yunchang_amd as Y
    import yunchang_amd.ring.utils as U
    from yunchang_amd.kernels import set_block_backend
    be = ShiftOracleBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    kv_recv = []                                    # ring ranks whose K/V (16-bit tensors) this rank received
    real_recv = U.RingComm.recv

    def recv(self, tensor, ring_rank):
        if tensor.dtype == torch.bfloat16:
            kv_recv.append(ring_rank % self.world_size)
        return real_recv(self, tensor, ring_rank)
    U.RingComm.recv = recv
    q, k, v, do = _inputs(ws)
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    loc = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in (q, k, v, do)]
    attn = Y.LongContextAttention(ring_impl_type="basic")
    res = {"refused": [], "cases": []}
    os.environ.pop("USP_RING_WINDOW", None)
    try:
        attn(*loc[:3], causal=True, window_size=(40, 0))
    except NotImplementedError as e:
        res["refused"].append("USP_RING_WINDOW=global" in str(e))
    os.environ["USP_RING_WINDOW"] = "global"
    for layer in (Y.LongContextAttention(ring_impl_type="zigzag"), Y.AsyncLongContextAttention(ring_impl_type="basic")):
        try:
            layer(*loc[:3], causal=True, window_size=(40, 0))
        except NotImplementedError as e:
            res["refused"].append("basic" in str(e))
    for win, causal in CASES:
        lq, lk, lv = (t.detach().clone().requires_grad_(True) for t in loc[:3])
        del be.launches[:], kv_recv[:]
        out = attn(lq, lk, lv, causal=causal, window_size=win)
        fwd, fwd_recv = list(be.launches), list(kv_recv)
        del be.launches[:], kv_recv[:]
        out.backward(loc[3])
        res["cases"].append(dict(got=[t.detach().float().numpy() for t in (out, lq.grad, lk.grad, lv.grad)],
                                 fwd=fwd, fwd_recv=fwd_recv, bwd=list(be.launches), bwd_recv=list(kv_recv)))
    if ud == 1:                                      # the ring function itself, and its packed forms
        win, causal = CASES[1]
        o1 = Y.ring_flash_attn_func(*loc[:3], causal=causal, window_size=win, group=Y.PROCESS_GROUP.RING_PG)
        o2 = Y.ring_flash_attn_kvpacked_func(loc[0], torch.stack(loc[1:3], dim=2), causal=causal, window_size=win,
                                             group=Y.PROCESS_GROUP.RING_PG)
        res["func"] = [o1.float().numpy(), o2.float().numpy()]
    return res


def _truth(ws, win, causal):
    q, k, v, do = _inputs(ws)
    o, l = shift_ref.ref_fwd(q, k, v, D ** -0.5, causal, win)
    return (o,) + shift_ref.ref_bwd(do, q, k, v, o.to(torch.bfloat16), l, D ** -0.5, causal, win)


@pytest.mark.parametrize("ws,ud,rd", [(2, 1, 2), (4, 1, 4), (4, 2, 2)])
def test_global_window_ring_on_gloo(ws, ud, rd):
    import yunchang_amd as Y
    from yunchang_amd.ring.window_blocks import WindowPlan
    res = run_distributed(_ring_worker, ws, ud, rd)
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    c = 64 * ws // rd
    for rank in range(ws):
        assert res[rank]["refused"] == [True, True, True], res[rank]["refused"]
        r = rank // ud                                                # ring rank (Ulysses groups are consecutive ranks)
        for (win, causal), case in zip(CASES, res[rank]["cases"]):
            what = f"grid {ud}x{rd} rank {rank} window {win} causal {causal}"
            truth = [ext(t, rank, world_size=ws, rd=rd, ud=ud) for t in _truth(ws, win, causal)]
            for got, want, name in zip(case["got"], truth, ("out", "dq", "dk", "dv")):
                tol = TOL["bfloat16"]["out"] if name == "out" else grad_tol("bfloat16", HQ // HKV)
                assert_close(got, want, *tol, f"{what} {name}")
            # exactly the planner's non-empty blocks, in step order; first launch adopts, last one finalises every row
            plan = WindowPlan(rd, c, causal, win[0], win[1], r)
            blocks = [plan.block(s) for s in plan.steps]
            assert [x[1:4] for x in case["fwd"]] == [(b.causal, b.window, b.shift) for b in blocks], what
            assert [x[4] for x in case["fwd"]] == [i > 0 for i in range(len(blocks))], what
            assert [x[5:] for x in case["fwd"]] == [(0, 0)] * (len(blocks) - 1) + [(0, c)], what
            assert [x[1:4] for x in case["bwd"]] == [(b.causal, b.window, b.shift) for b in blocks], what
            assert [x[4] for x in case["bwd"]] == [i > 0 for i in range(len(blocks))], what
            # K and V of the non-empty steps' source ranks, and of no other
            want_src = sorted((r - s) % rd for s in plan.recv)
            assert sorted(case["fwd_recv"]) == sorted(want_src * 2) and sorted(case["bwd_recv"]) == sorted(want_src * 2), what
            assert len(plan.steps) < rd or rd == 2 or win[0] < 0, "the cases are meant to have empty blocks"
        if ud == 1:
            o = ext(_truth(ws, *CASES[1])[0], rank, world_size=ws, rd=rd, ud=ud)
            for got in res[rank]["func"]:
                assert_close(got, o, *TOL["bfloat16"]["out"], f"ring_flash_attn_func rank {rank}")


# ---- 4. ring degree 1: the switch changes nothing --------------------------------------------------------------------------------
def _degree1_worker(rank, ws):
    import yunchang_amd as Y
    from yunchang_amd.kernels import set_block_backend
    set_block_backend(OracleBlockBackend())
    Y.set_seq_parallel_pg(ws, 1, rank, ws)
    q, k, v, do = _inputs(ws)
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    loc = [ext(t, rank, world_size=ws, rd=1, ud=ws).detach().clone() for t in (q, k, v, do)]
    attn = Y.LongContextAttention(ring_impl_type="basic")
    runs = []
    for mode in (None, "global"):
        os.environ.pop("USP_RING_WINDOW", None)
        if mode:
            os.environ["USP_RING_WINDOW"] = mode
        lq, lk, lv = (t.detach().clone().requires_grad_(True) for t in loc[:3])
        out = attn(lq, lk, lv, causal=True, window_size=(40, 0))
        out.backward(loc[3])
        runs.append([out.detach(), lq.grad, lk.grad, lv.grad])
    return all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("ws", [1, 2])
def test_ring_degree_one_is_untouched_by_the_switch(ws):
    assert all(run_distributed(_degree1_worker, ws))


def test_relay_of_unrequested_step_raises():
    """KVRelay with step sets: no slot, no event for a step that was not requested (ring degree 1 stands in: nothing is posted)."""
    from yunchang_amd.ring.utils import KVRelay

    class OneRank:
        @staticmethod
        def get_world_size(g=None):
            return 1

        @staticmethod
        def get_rank(g=None):
            return 0
    import yunchang_amd.ring.utils as U
    real, U.dist = U.dist, OneRank
    try:
        k = torch.zeros(1, 4, 1, 8)
        with KVRelay(None, k, k, recv_steps=[], send_steps=[]) as relay:
            assert relay.get(0)[0] is k
            with pytest.raises(RuntimeError):
                relay.get(1)
    finally:
        U.dist = real
