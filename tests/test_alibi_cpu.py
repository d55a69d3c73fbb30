"""ALiBi (alibi_slopes) without a GPU: the fp64 reference against torch autograd of the written-out formula, what the C ABI
refuses before any launch (usp_flash_fwd_alibi / usp_flash_bwd_alibi), the Python refusals and slope-shape checks, and the
schedules -- Ulysses head slices, the basic ring's per-step diagonal shift under USP_RING_ALIBI=global, a 2 x 2 grid, the
global window beside it -- on gloo ranks with an ALiBi-aware numpy block backend, against the unsharded fp64 reference."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import alibi_ref
from dist_util import run_distributed
from golden_util import TOL, assert_close, grad_tol
from oracle_backend import OracleBlockBackend, _np, _operand, _put

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the reference against autograd of the written-out formula -------------------------------------------------------------
@pytest.mark.parametrize("Sq,Sk,causal,window,shift,two_d", [(24, 40, False, None, 0, True), (40, 24, True, None, 16, False),
                                                             (32, 32, False, (9, 4), 0, True), (24, 40, True, (12, 0), 7, True),
                                                             (24, 40, False, None, -11, False)])
def test_reference_against_autograd(Sq, Sk, causal, window, shift, two_d):
    B, Hq, Hkv, D = 2, 4, 2, 16
    g = torch.Generator().manual_seed(3)
    q, k, v, do = (torch.randn(B, s, h, D, generator=g, dtype=torch.float64) for s, h in ((Sq, Hq), (Sk, Hkv), (Sk, Hkv), (Sq, Hq)))
    m = alibi_ref.default_slopes(Hq)
    assert torch.allclose(m, torch.tensor([0.25, 0.0625, 0.015625, 0.00390625]))
    if two_d:
        m = torch.stack([m, m.flip(0)])
    scale = 0.3
    out, lse, dq, dk, dv = alibi_ref.ref_bwd(do, q, k, v, scale, m, causal, window, shift)
    # the formula of include/usp_hip.h, written out with loops over (b, h) and plain softmax; autograd differentiates it
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    m2 = (m if m.dim() == 2 else m[None].expand(B, Hq)).double()
    i = torch.arange(Sq)[:, None] + (Sk - Sq + shift)
    j = torch.arange(Sk)[None, :]
    left, right = (-1, -1) if window is None else window
    right = 0 if causal else right
    vis = torch.ones(Sq, Sk, dtype=torch.bool)
    if right >= 0:
        vis &= j <= i + right
    if left >= 0:
        vis &= j >= i - left
    assert bool(vis.any(1).all()), "the cases keep every row alive (softmax of an empty row is NaN in the plain formula)"
    outs, lses = [], []
    for b in range(B):
        per_head = []
        for h in range(Hq):
            s = scale * ql[b, :, h] @ kl[b, :, h // (Hq // Hkv)].T - m2[b, h] * (i - j).abs()
            s = s.masked_fill(~vis, float("-inf"))
            per_head.append(torch.softmax(s, -1) @ vl[b, :, h // (Hq // Hkv)])
            lses.append(torch.logsumexp(s, -1))
        outs.append(torch.stack(per_head, 1))
    o2 = torch.stack(outs)
    o2.backward(do)
    assert torch.allclose(out, o2.detach(), atol=1e-12, rtol=1e-10)
    assert torch.allclose(lse.reshape(-1, Sq), torch.stack(lses).detach(), atol=1e-12, rtol=1e-10)
    for got, want in ((dq, ql.grad), (dk, kl.grad), (dv, vl.grad)):
        assert torch.allclose(got, want, atol=1e-11, rtol=1e-9)
    # slopes = None is the unbiased function (tests/shift_ref.py)
    import shift_ref
    o0, l0 = alibi_ref.ref_fwd(q, k, v, scale, None, causal, window, shift)
    o1, l1 = shift_ref.ref_fwd(q, k, v, scale, causal, window, shift)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)


# ---- 2. the C ABI at the host: what is refused before any launch ------------------------------------------------------------------
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


def test_abi_feature_bit_entry_points_and_unchanged_structs():
    _C, L = _lib()
    txt = open(os.path.join(ROOT, "include", "usp_hip.h")).read()
    assert _C.USP_ATTN_ALIBI == 256 == int(re.search(r"#define USP_ATTN_ALIBI (\d+)", txt).group(1))
    assert L.usp_attn_features() & _C.USP_ATTN_ALIBI
    assert L.usp_attn_features() & (_C.USP_ATTN_WINDOW | _C.USP_ATTN_SOFTCAP | _C.USP_ATTN_SHIFT) == 2 | 64 | 128
    assert L.usp_abi_version() == 7 == _C.ABI_VERSION
    for name in ("usp_flash_fwd_alibi", "usp_flash_bwd_alibi"):
        # looked up on first use, behind the feature bit: a library built before them must still load
        assert name in _C.ALIBI_EXPORTS and name in _C.EXPORTS and hasattr(L, name)
        fn = _C._alibi_entry(name)
        assert fn.restype is ctypes.c_int and fn.argtypes[1:] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        assert re.search(r"int " + name + r"\(const usp_(fwd|bwd)_args\* args, const float\* alibi_slopes, int64_t alibi_stride_b, "
                         r"void\* stream\);", txt), name
    for cls in (_C.UspFwdArgs, _C.UspBwdArgs):
        assert cls._fields_[-1] == ("softcap", ctypes.c_float)
    assert len(re.findall(r"typedef struct", txt)) == 3


def test_abi_declines_without_launch():
    """Host memory stands in for the device pointers (slopes included): every call below must return before anything is launched."""
    _C, L = _lib()
    buf = ctypes.create_string_buffer(1 << 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    seq = (ctypes.c_int32 * 2)(0, 16)
    slopes = (ctypes.c_float * 2)(0.5, 0.25)
    sp = ctypes.cast(slopes, ctypes.c_void_p)
    for cls, call in ((_C.UspFwdArgs, L.usp_flash_fwd_alibi), (_C.UspBwdArgs, L.usp_flash_bwd_alibi)):
        a = _args(_C, cls, addr)                       # softcap together with slopes
        a.flags, a.softcap = _C.USP_ATTN_SOFTCAP, 30.0
        assert call(ctypes.byref(a), sp, 0, None) == -2
        a = _args(_C, cls, addr)                       # a packed batch
        a.seq_q = a.seq_k = ctypes.addressof(seq)
        if cls is _C.UspBwdArgs:
            a.total_k = 16
        assert call(ctypes.byref(a), sp, 0, None) == -2
        a = _args(_C, cls, addr)                       # the 64-row family forced
        a.flags = _C.USP_FORCE_ROW64
        assert call(ctypes.byref(a), sp, 0, None) == -2
        a = _args(_C, cls, addr)                       # a negative batch stride
        assert call(ctypes.byref(a), sp, -2, None) == -1
        a.flags = _C.USP_FORCE_ROW64                   # ... comes before the declines
        assert call(ctypes.byref(a), sp, -2, None) == -1
        a = _args(_C, cls, addr)                       # the existing checks still come first
        a.flags, a.softmax_scale = _C.USP_FORCE_ROW64, 0.0
        assert call(ctypes.byref(a), sp, 0, None) == -1
        a = _args(_C, cls, addr)
        a.flags = _C.USP_FORCE_ROW64 | _C.USP_FORCE_WAVE32
        assert call(ctypes.byref(a), sp, 0, None) == -1
        assert L.usp_last_launch_kinds() == 0


# ---- 3. Python: refusals and the shapes of the slopes ----------------------------------------------------------------------------
def test_alibi_value_shapes_dtype_device():
    from yunchang_amd import _C
    cpu = torch.device("cpu")
    assert _C.alibi_value(None, 2, 4, cpu) is None
    t, sb = _C.alibi_value(torch.rand(4), 2, 4, cpu)
    assert sb == 0 and t.is_contiguous() and t.dtype == torch.float32
    t, sb = _C.alibi_value(torch.rand(4, 2).T, 2, 4, cpu)
    assert sb == 4 and t.is_contiguous() and tuple(t.shape) == (2, 4)
    for bad in (torch.rand(3), torch.rand(4, 2), torch.rand(2, 4, 1), torch.rand(1, 4), torch.rand(4).double(),
                torch.rand(4).to(torch.bfloat16), torch.rand(2, 4).to("meta"), [0.5] * 4):
        with pytest.raises(ValueError):
            _C.alibi_value(bad, 2, 4, cpu)


def test_python_refusals(monkeypatch):
    from yunchang_amd import _C
    from yunchang_amd.comm.all_to_all import local_alibi_slopes, local_heads
    from yunchang_amd.kernels import attention as KA
    from yunchang_amd.ring.ring_flash_attn_varlen import ring_flash_attn_varlen_func
    from yunchang_amd.ring.zigzag_ring_flash_attn_varlen import zigzag_ring_flash_attn_varlen_func
    q = torch.zeros(2, 16, 4, 64, dtype=torch.bfloat16)
    m = alibi_ref.default_slopes(4)
    # ALiBi together with softcap: no kernel holds both steps
    for call in (lambda: KA.hip_attn_func(q, q, q, softcap=30.0, alibi_slopes=m),
                 lambda: KA.hip_attn_forward(q, q, q, softcap=30.0, alibi_slopes=m),
                 lambda: KA.hip_attn_backward(q, q, q, q, q, None, q, q, q, softcap=30.0, alibi_slopes=m),
                 lambda: KA.get_block_backend(softcap=30.0, alibi=m)):
        with pytest.raises(NotImplementedError, match="softcap"):
            call()
    # the wrong shape is a ValueError before anything touches a device
    with pytest.raises(ValueError):
        KA.hip_attn_forward(q, q, q, alibi_slopes=torch.rand(5))
    # the wrapper: dense calls carry the slopes, packed ones refuse
    seen = {}

    class Rec:
        def fwd(self, *a, **kw):
            seen["fwd"] = kw

        def bwd(self, *a, **kw):
            seen["bwd"] = kw

        def merge(self):
            return "merge"
    prev = KA.set_block_backend(Rec())
    try:
        be = KA.get_block_backend(alibi=m)
        be.fwd(1, shift=5)
        be.bwd(2)
        assert seen["fwd"] == {"alibi": m, "shift": 5} and seen["bwd"] == {"alibi": m} and be.merge() == "merge"
        for packed in (be.fwd_packed, be.bwd_packed):
            with pytest.raises(NotImplementedError, match="packed"):
                packed()
        assert isinstance(KA.get_block_backend(), Rec)
    finally:
        KA.set_block_backend(prev)
    # the packed rings say which ring serves it
    t3 = torch.zeros(32, 4, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 32], dtype=torch.int32)
    for f in (ring_flash_attn_varlen_func, zigzag_ring_flash_attn_varlen_func):
        with pytest.raises(NotImplementedError, match="basic"):
            f(t3, t3, t3, cu, 32, causal=True, alibi_slopes=m)
    # the head map of the exchange, and the slopes cut by it
    assert local_heads(8, 4, 3) == slice(6, 8)
    m8 = alibi_ref.default_slopes(8)
    assert torch.equal(local_alibi_slopes(m8, 8, 4, 1), m8[2:4])
    assert torch.equal(local_alibi_slopes(torch.stack([m8, m8.flip(0)]), 8, 2, 1), torch.stack([m8, m8.flip(0)])[:, 4:])
    assert local_alibi_slopes(m8[:2], 8, 4, 1) is not None and torch.equal(local_alibi_slopes(m8[:2], 8, 4, 1), m8[:2])
    assert local_alibi_slopes(None, 8, 4, 1) is None and local_alibi_slopes(m8, 8, 1, 0) is m8
    for bad in (m8[:3], torch.rand(2, 5), torch.rand(1, 2, 8)):
        with pytest.raises(ValueError):
            local_alibi_slopes(bad, 8, 4, 1)

    # a library without the feature bit
    class Old:
        @staticmethod
        def usp_attn_features():
            return _C.USP_ATTN_WINDOW | _C.USP_ATTN_SOFTCAP | _C.USP_ATTN_SHIFT
    monkeypatch.setattr(_C, "load", lambda: Old)
    with pytest.raises(NotImplementedError, match="rebuild it"):
        _C._alibi_entry("usp_flash_fwd_alibi")


# ---- 4. the schedules on gloo ------------------------------------------------------------------------------------------------------
def _np_scores(q, k, scale, slopes, causal, window, shift):
    """(B,Hq,Sq,Sk) fp64 numpy: scale q k^T - m |i + off - j|, -inf outside the mask; written on its own (not alibi_ref)."""
    qn, kn = _np(q), _np(k)
    B, Sq, Hq, _ = qn.shape
    Sk = kn.shape[1]
    kn = np.repeat(kn, Hq // kn.shape[2], axis=2)
    off = Sk - Sq + (shift or 0)
    rel = np.arange(Sq)[:, None] + off - np.arange(Sk)[None, :]            # i + off - j
    s = np.einsum("bihd,bjhd->bhij", qn, kn) * scale
    if slopes is not None:
        m = slopes.detach().double().numpy()
        m = np.broadcast_to(m, (B, Hq)) if m.ndim == 1 else m
        assert m.shape == (B, Hq), (m.shape, B, Hq)
        s = s - m[:, :, None, None] * np.abs(rel)[None, None]
    left, right = (-1, -1) if window is None else window
    right = 0 if causal else right
    vis = np.ones((Sq, Sk), dtype=bool)
    if right >= 0:
        vis &= rel >= -right
    if left >= 0:
        vis &= rel <= left
    return np.where(vis[None, None], s, -np.inf)


class AlibiNumpyBackend(OracleBlockBackend):
    """The block seam in numpy fp64 with `alibi`, `shift` and `window`; logs ("fwd" | "bwd", causal, window, shift, heads of the
    slopes, merge_in | accum_dq)."""

    def __init__(self):
        super().__init__()
        self.launches = []

    def fwd(self, q, k, v, softmax_scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None,
            window=None, k_splits=None, shift=None, alibi=None):
        Sq = q.shape[1]
        fe = Sq if final_end is None else final_end
        for t, what in ((q, "q"), (k, "k"), (v, "v"), (acc, "acc")):
            _operand(t, what)
        _operand(out, "out", 8, 8)
        assert (fe <= final_begin or out is not None) and ((final_begin <= 0 and fe >= Sq) or acc is not None) \
            and (not merge_in or acc is not None), "final rows need `out`, the others (and a merge) need `acc`"
        assert alibi is None or (alibi.dtype == torch.float32 and alibi.shape[-1] == q.shape[2])
        self.launches.append(("fwd", bool(causal), window, shift, None if alibi is None else tuple(alibi.shape), bool(merge_in)))
        s = _np_scores(q, k, softmax_scale, alibi, causal, window, shift)
        with np.errstate(invalid="ignore", divide="ignore"):
            mx = s.max(-1)
            safe = np.where(np.isfinite(mx), mx, 0.0)
            e = np.exp(s - safe[..., None])
            bl = np.where(np.isfinite(mx), safe + np.log(e.sum(-1)), -np.inf)                 # (B,H,Sq)
            p = np.where(np.isfinite(bl)[..., None], np.exp(s - np.where(np.isfinite(bl), bl, 0.0)[..., None]), 0.0)
            bo = np.einsum("bhij,bjhd->bihd", p, np.repeat(_np(v), q.shape[2] // v.shape[2], axis=2))
            if merge_in:
                old = _np(lse)
                new = np.logaddexp(old, bl)
                fin = np.isfinite(new)
                w_old = np.where(fin, np.exp(old - np.where(fin, new, 0.0)), 0.0)
                w_blk = np.where(fin, np.exp(bl - np.where(fin, new, 0.0)), 0.0)
                bo = _np(acc) * np.swapaxes(w_old, 1, 2)[..., None] + bo * np.swapaxes(w_blk, 1, 2)[..., None]
                bl = new
        _put(lse, bl)
        if fe > final_begin:
            _put(out[:, final_begin:fe], bo[:, final_begin:fe])
        if final_begin > 0:
            _put(acc[:, :final_begin], bo[:, :final_begin])
        if fe < Sq:
            _put(acc[:, fe:], bo[:, fe:])

    def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale, causal, accum_dq=False, accum_dk=False, accum_dv=False,
            dq16=None, dk16=None, dv16=None, window=None, only=None, shift=None, alibi=None):
        assert only is None
        for t, what in ((dout, "dout"), (q, "q"), (k, "k"), (v, "v"), (dq, "dq"), (dk, "dk"), (dv, "dv")):
            _operand(t, what)
        self.launches.append(("bwd", bool(causal), window, shift, None if alibi is None else tuple(alibi.shape), bool(accum_dq)))
        B, Sq, Hq, D = q.shape
        Sk, Hkv = k.shape[1], k.shape[2]
        g = Hq // Hkv
        s = _np_scores(q, k, softmax_scale, alibi, causal, window, shift)
        ln, dl, don, qn = _np(lse), _np(delta), _np(dout), _np(q)
        fin = np.isfinite(ln)
        with np.errstate(invalid="ignore"):
            p = np.where(fin[..., None], np.exp(s - np.where(fin, ln, 0.0)[..., None]), 0.0)
        vv, kk = np.repeat(_np(v), g, axis=2), np.repeat(_np(k), g, axis=2)
        ds = p * (np.einsum("bihd,bjhd->bhij", don, vv) - dl[..., None]) * softmax_scale
        grads = (np.einsum("bhij,bjhd->bihd", ds, kk),
                 np.einsum("bhij,bihd->bjhd", ds, qn).reshape(B, Sk, Hkv, g, D).sum(3),
                 np.einsum("bhij,bihd->bjhd", p, don).reshape(B, Sk, Hkv, g, D).sum(3))
        for val, dst, d16, accum in zip(grads, (dq, dk, dv), (dq16, dk16, dv16), (accum_dq, accum_dk, accum_dv)):
            tot = val + _np(dst) if accum else val
            _put(d16 if d16 is not None else dst, tot)


B, HQ, HKV, D, CH = 2, 4, 2, 32, 48       # CH rows per rank
WINDOWED = [(True, (70, 0)), (False, (60, 55))]      # (causal, window) at ring degree 4; the second: blocks behind the queries
                                                     # (negative shifts) under a right bound
SCALE = D ** -0.5


def _inputs(ws):
    g = torch.Generator().manual_seed(11)
    return [torch.randn(B, CH * ws, h, D, generator=g).to(torch.bfloat16) for h in (HQ, HKV, HKV, HQ)]


def _slopes(kind):
    m = alibi_ref.default_slopes(HQ)
    return torch.stack([m, m.flip(0)]) if kind == "2d" else m


_TRUTH = {}


def _truth(ws, kind, causal, window=None):
    key = (ws, kind, causal, window)
    if key not in _TRUTH:
        q, k, v, do = _inputs(ws)
        r = alibi_ref.ref_bwd(do, q, k, v, SCALE, _slopes(kind), causal, window, 0, out_dtype=torch.bfloat16)
        _TRUTH[key] = (r[0],) + r[2:]
    return _TRUTH[key]


def _run_layer(layer, loc, slopes, **kw):
    lq, lk, lv = (t.detach().clone().requires_grad_(True) for t in loc[:3])
    out = layer(lq, lk, lv, alibi_slopes=slopes, **kw)
    out.backward(loc[3])
    return [t.detach().float().numpy() for t in (out, lq.grad, lk.grad, lv.grad)]


def _worker(rank, ws, ud, rd, ulysses_layer):
    import torch.distributed as dist
    import yunchang_amd as Y
    from yunchang_amd.comm.all_to_all import local_heads
    from yunchang_amd.kernels import set_block_backend
    be = AlibiNumpyBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    loc = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in _inputs(ws)]
    res = {"refused": [], "cases": {}, "launches": {}}
    os.environ.pop("USP_RING_WINDOW", None)
    os.environ.pop("USP_RING_ALIBI", None)
    if ulysses_layer:                               # UlyssesAttention over the whole world: full, (B, Hq) and local-head slopes
        layer = Y.UlyssesAttention(dist.group.WORLD)
        u = dist.get_rank()
        for name, m in (("full", _slopes("1d")), ("2d", _slopes("2d")), ("local", _slopes("1d")[local_heads(HQ, ws, u)]),
                        ("local2d", _slopes("2d")[:, local_heads(HQ, ws, u)])):
            res["cases"][name] = _run_layer(layer, loc, m, causal=True)
        try:
            _run_layer(layer, loc, torch.rand(3), causal=True)
        except ValueError:
            res["refused"].append(True)
        return res
    attn = Y.LongContextAttention(ring_impl_type="basic")
    if rd > 1:                                      # the default refuses and names the switch
        try:
            attn(*loc[:3], causal=True, alibi_slopes=_slopes("1d"))
        except NotImplementedError as e:
            res["refused"].append("USP_RING_ALIBI=global" in str(e) and "different function" in str(e))
    os.environ["USP_RING_ALIBI"] = "global"
    if rd > 1:                                      # the zigzag and stripe rings and the async layer point at the basic ring
        for layer in (Y.LongContextAttention(ring_impl_type="zigzag"), Y.LongContextAttention(ring_impl_type="strip"),
                      Y.AsyncLongContextAttention(ring_impl_type="basic")):
            try:
                layer(*loc[:3], causal=True, alibi_slopes=_slopes("1d"))
            except NotImplementedError as e:
                res["refused"].append("basic" in str(e))
    for kind, causal in (("1d", True), ("2d", False), ("2d", True)):
        del be.launches[:]
        res["cases"][(kind, causal, None)] = _run_layer(attn, loc, _slopes(kind), causal=causal)
        res["launches"][(kind, causal, None)] = list(be.launches)
    if rd == 4:                                     # together with the global window: the planner's blocks carry the same shift
        os.environ["USP_RING_WINDOW"] = "global"
        for causal, win in WINDOWED:
            del be.launches[:]
            res["cases"][("2d", causal, win)] = _run_layer(attn, loc, _slopes("2d"), causal=causal, window_size=win)
            res["launches"][("2d", causal, win)] = list(be.launches)
    if rd == 1 and ud == 1:                         # ring degree 1: every dense ring is one block, with or without the switch
        os.environ.pop("USP_RING_ALIBI", None)
        for impl in ("basic", "zigzag", "strip"):
            del be.launches[:]
            res["cases"][impl] = _run_layer(Y.LongContextAttention(ring_impl_type=impl), loc, _slopes("2d"), causal=True)
            res["launches"][impl] = list(be.launches)
    return res


def _check(res, ws, ud, rd, name, kind, causal, window=None):
    import yunchang_amd as Y
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    for rank in range(ws):
        truth = [ext(t, rank, world_size=ws, rd=rd, ud=ud) for t in _truth(ws, kind, causal, window)]
        for got, want, what in zip(res[rank]["cases"][name], truth, ("out", "dq", "dk", "dv")):
            tol = TOL["bfloat16"]["out"] if what == "out" else grad_tol("bfloat16", HQ // HKV)
            assert_close(got, want, *tol, f"grid {ud}x{rd} rank {rank} {name} {what}")


def test_ulysses_slices_the_slopes():
    res = run_distributed(_worker, 2, 2, 1, True)
    for name, kind in (("full", "1d"), ("2d", "2d"), ("local", "1d"), ("local2d", "2d")):
        _check(res, 2, 2, 1, name, kind, True)
    assert all(r["refused"] == [True] for r in res)


@pytest.mark.parametrize("ws,ud,rd", [(2, 1, 2), (4, 1, 4), (4, 2, 2)])
def test_global_alibi_on_the_basic_ring(ws, ud, rd):
    res = run_distributed(_worker, ws, ud, rd, False)
    c = CH * ws // rd
    for rank in range(ws):
        assert res[rank]["refused"] == [True] * 4, res[rank]["refused"]
    for kind, causal in (("1d", True), ("2d", False), ("2d", True)):
        _check(res, ws, ud, rd, (kind, causal, None), kind, causal)
        for rank in range(ws):
            r = rank // ud                          # ring rank (Ulysses groups are consecutive ranks)
            steps = [s for s in range(rd) if not (causal and s > r)]
            # (r - kr) * S: negative behind the queries; the rank's own block is an unshifted launch (no keyword)
            want = [(r - (r - s) % rd) * c or None for s in steps]
            heads = ((B, HQ // ud) if kind == "2d" else (HQ // ud,))
            for tag in ("fwd", "bwd"):
                got = [x for x in res[rank]["launches"][(kind, causal, None)] if x[0] == tag]
                assert [x[3] for x in got] == want, (rank, tag, got)
                assert [x[1] for x in got] == [causal and s == 0 for s in steps]
                assert all(x[4] == heads for x in got) and [x[5] for x in got] == [i > 0 for i in range(len(steps))]
            assert causal or r == rd - 1 or any(w is not None and w < 0 for w in want)     # (the last ring rank has every key in front of it)
    if rd == 4:
        from yunchang_amd.ring.window_blocks import WindowPlan
        for causal, win in WINDOWED:
            _check(res, ws, ud, rd, ("2d", causal, win), "2d", causal, win)
            for rank in range(ws):
                r = rank // ud
                plan = WindowPlan(rd, c, causal, win[0], win[1], r)
                want = [(r - (r - s) % rd) * c or None for s in plan.steps]    # the planner's non-empty blocks, the bias's shift
                for tag in ("fwd", "bwd"):
                    got = [x for x in res[rank]["launches"][("2d", causal, win)] if x[0] == tag]
                    assert [x[3] for x in got] == want, (rank, tag, got, want)
                assert causal or r == rd - 1 or any(w is not None and w < 0 for w in want), (rank, want)
        assert [len(WindowPlan(4, c, True, 70, 0, r).steps) for r in range(4)] == [1, 2, 3, 3]


def test_ring_degree_one_is_one_block():
    res = run_distributed(_worker, 1, 1, 1, False)
    for name in (("1d", True, None), ("2d", False, None), ("2d", True, None)):
        _check(res, 1, 1, 1, name, name[0], name[1])
    for impl in ("basic", "zigzag", "strip"):
        _check(res, 1, 1, 1, impl, "2d", True)
        assert [x[0] for x in res[0]["launches"][impl]] == ["fwd", "bwd"], res[0]["launches"][impl]
