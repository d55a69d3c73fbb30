"""Logit soft-capping (flash-attn's `softcap`) -- the CPU side: the fp64 reference every softcap test compares against, its
cross-check against torch autograd, the C ABI's argument checks (no launch), the Python refusals, and the ring / USP
schedules on gloo ranks with a softcap-aware numpy block backend.

Semantics (flash-attn's, which the reference forwards unchanged to every block call,
yunchang/ring/zigzag_ring_flash_attn.py:29-43 and :115-137):
    S = scale * q k^T ;  S' = cap * tanh(S / cap)  (replaces S; the causal / window / ragged mask is applied to S')
    lse = logsumexp_j S' ;  out = softmax(S') v
    dS' = P * (dP - delta) ;  dS = dS' * (1 - tanh^2(S / cap)) * scale ;  dQ = dS K ;  dK = dS^T Q
There is no reference-produced golden (the reference's TORCH path ignores softcap and flash-attn is not installed): the
restatement below is the oracle, and test_reference_matches_torch_autograd ties it to autograd of the formula.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dist_util import run_distributed  # noqa: E402


# ---- fp64 reference ---------------------------------------------------------------------------------------------------
def _ein(spec, *ops):
    """np.einsum in fp64 through torch's batched GEMMs (numpy's loops would eat the GPU file's time budget)."""
    return torch.einsum(spec, *(torch.from_numpy(np.ascontiguousarray(o, dtype=np.float64)) for o in ops)).numpy()


def _mask(Sq, Sk, causal, window):
    """(Sq, Sk) bool: key j visible to query i (bottom-right aligned, flash-attn's window (left, right))."""
    left, right = (-1, -1) if window is None else window
    if causal:
        right = 0
    row = np.arange(Sq)[:, None] + (Sk - Sq)
    col = np.arange(Sk)[None, :]
    vis = np.ones((Sq, Sk), dtype=bool)
    if right >= 0:
        vis &= col <= row + right
    if left >= 0:
        vis &= col >= row - left
    return vis


def _scores(q, k, scale, cap, causal, window):
    """-> (capped masked scores S' (B,Hq,Sq,Sk), t = tanh(S / cap) or None, visibility mask)."""
    g = q.shape[2] // k.shape[2]
    s = _ein("bthd,bshd->bhts", q, np.repeat(k, g, axis=2)) * scale
    t = None
    if cap:
        t = np.tanh(s / cap)
        s = cap * t
    vis = _mask(q.shape[1], k.shape[1], causal, window)
    return np.where(vis, s, -np.inf), t, vis


def ref_fwd(q, k, v, scale, cap, causal=False, window=None):
    """fp64: (out (B,Sq,Hq,D), lse (B,Hq,Sq)); empty rows give out 0, lse -inf.  cap None / 0 = off."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    s, _, _ = _scores(q, k, scale, cap, causal, window)
    m = s.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    p = np.exp(s - m)
    l = p.sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = (m + np.log(l))[..., 0]
        att = np.where(l > 0, p / l, 0.0)
    g = q.shape[2] // k.shape[2]
    return _ein("bhts,bshd->bthd", att, np.repeat(v, g, axis=2)), lse


def ref_bwd_from(dout, q, k, v, lse, delta, scale, cap, causal=False, window=None):
    """fp64 block backward given the GLOBAL lse / delta (B,Hq,Sq) -- the block contract of the ring schedules."""
    dout, q, k, v, lse, delta = (np.asarray(x, np.float64) for x in (dout, q, k, v, lse, delta))
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    g = Hq // Hkv
    s, t, vis = _scores(q, k, scale, cap, causal, window)
    fin = np.isfinite(lse)
    p = np.where(vis & fin[..., None], np.exp(s - np.where(fin, lse, 0.0)[..., None]), 0.0)
    vv, kk = np.repeat(v, g, axis=2), np.repeat(k, g, axis=2)
    dv = _ein("bhts,bthd->bshd", p, dout).reshape(B, Sk, Hkv, g, D).sum(3)
    dp = _ein("bthd,bshd->bhts", dout, vv)
    ds = p * (dp - delta[..., None])
    if cap:
        ds = ds * (1.0 - t * t)
    ds = ds * scale
    dq = _ein("bhts,bshd->bthd", ds, kk)
    dk = _ein("bhts,bthd->bshd", ds, q).reshape(B, Sk, Hkv, g, D).sum(3)
    return dq, dk, dv


def ref_bwd(dout, q, k, v, scale, cap, causal=False, window=None):
    """fp64 (dq, dk, dv) of one whole attention call."""
    out, lse = ref_fwd(q, k, v, scale, cap, causal, window)
    delta = _ein("bshd,bshd->bhs", np.asarray(dout, np.float64), out)
    return ref_bwd_from(dout, q, k, v, lse, delta, scale, cap, causal, window)


def assert_cap_bites(q, k, v, dout, scale, cap, causal, window, tol_out, tol_grad):
    """A parity case shows softcap only if the capped reference differs from the uncapped one by far more than the
    tolerance it is checked at (10x), in the output and in every gradient."""
    o1, _ = ref_fwd(q, k, v, scale, cap, causal, window)
    o0, _ = ref_fwd(q, k, v, scale, None, causal, window)
    g1 = ref_bwd(dout, q, k, v, scale, cap, causal, window)
    g0 = ref_bwd(dout, q, k, v, scale, None, causal, window)
    assert np.abs(o1 - o0).max() > 10 * tol_out, "softcap does not change the output enough for the case to show it"
    for a, b, nm in zip(g1, g0, ("dq", "dk", "dv")):
        assert np.abs(a - b).max() > 10 * tol_grad, f"softcap does not change {nm} enough for the case to show it"


def make_case(B, Sq, Sk, Hq, Hkv, D, dtype=torch.bfloat16, q_mul=4.0, seed=0, device="cpu"):
    """N(0,1) inputs with q scaled up (q_mul) so that a cap of a few units bites: scale * |q k| reaches ~10."""
    gen = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, Sq, Hq, D, generator=gen) * q_mul).to(dtype)
    k, v = (torch.randn(B, Sk, Hkv, D, generator=gen).to(dtype) for _ in range(2))
    do = torch.randn(B, Sq, Hq, D, generator=gen).to(dtype)
    return tuple(t.to(device) for t in (q, k, v, do))


def np64(t):
    return t.detach().cpu().to(torch.float64).numpy()


# ---- the reference against autograd --------------------------------------------------------------------------------------
def _torch_ref(q, k, v, scale, cap, causal, window):
    g = q.shape[2] // k.shape[2]
    kk, vv = k.repeat_interleave(g, dim=2), v.repeat_interleave(g, dim=2)
    s = torch.einsum("bthd,bshd->bhts", q, kk) * scale
    s = cap * torch.tanh(s / cap)
    vis = torch.from_numpy(_mask(q.shape[1], k.shape[1], causal, window))
    s = s.masked_fill(~vis, float("-inf"))
    return torch.einsum("bhts,bshd->bthd", torch.softmax(s, -1), vv)


@pytest.mark.parametrize("Sq,Sk,Hq,Hkv,causal,window", [(24, 40, 4, 2, True, None), (32, 32, 2, 2, False, (5, 3)),
                                                        (16, 48, 8, 2, False, None), (40, 40, 4, 1, True, (7, -1))])
def test_reference_matches_torch_autograd(Sq, Sk, Hq, Hkv, causal, window):
    """The numpy restatement (forward and the tanh' chain of its backward) against torch.float64 autograd of
    cap*tanh(scale q k^T / cap) + masked softmax: causal bottom-right alignment (Sq != Sk), a window, GQA."""
    q, k, v, do = (t.double() for t in make_case(1, Sq, Sk, Hq, Hkv, 16, torch.float64, seed=3))
    scale, cap = 16 ** -0.5, 2.5
    qt, kt, vt = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = _torch_ref(qt, kt, vt, scale, cap, causal, window)
    out.backward(do)
    o, _ = ref_fwd(q.numpy(), k.numpy(), v.numpy(), scale, cap, causal, window)
    grads = ref_bwd(do.numpy(), q.numpy(), k.numpy(), v.numpy(), scale, cap, causal, window)
    np.testing.assert_allclose(o, out.detach().numpy(), atol=1e-10, rtol=1e-10)
    for a, b in zip(grads, (qt.grad, kt.grad, vt.grad)):
        np.testing.assert_allclose(a, b.numpy(), atol=1e-10, rtol=1e-10)
    assert_cap_bites(q.numpy(), k.numpy(), v.numpy(), do.numpy(), scale, cap, causal, window, 2e-2, 5e-2)


# ---- C ABI: what is refused before any launch ---------------------------------------------------------------------------------
def _lib():
    from yunchang_amd import _C
    if not os.path.exists(_C.lib_path()):
        pytest.fail("libusp_hip.so is not built: run __graft_entry__.build() first")
    return _C, _C.load()


def _header_define(name):
    import re
    txt = open(os.path.join(ROOT, "include", "usp_hip.h")).read()
    return int(re.search(rf"#define {name} (\d+)", txt).group(1))


def test_abi_reports_softcap():
    _C, L = _lib()
    assert _C.USP_ATTN_SOFTCAP == 64 == _header_define("USP_ATTN_SOFTCAP")
    assert L.usp_attn_features() & _C.USP_ATTN_SOFTCAP
    assert L.usp_attn_features() & _C.USP_ATTN_WINDOW
    assert L.usp_abi_version() == 7
    assert _C.UspFwdArgs._fields_[-1] == ("softcap", ctypes.c_float)
    assert _C.UspBwdArgs._fields_[-1] == ("softcap", ctypes.c_float)


def _valid_fwd(_C, addr):
    a = _C.UspFwdArgs()
    a.dtype, a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D = 0, 1, 16, 16, 2, 2, 64
    a.softmax_scale = 0.125
    a.lse = addr
    return a


def _valid_bwd(_C, addr):
    a = _C.UspBwdArgs()
    a.dtype, a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D = 0, 1, 16, 16, 2, 2, 64
    a.softmax_scale = 0.125
    a.lse = a.delta = addr
    return a


def test_abi_rejects_bad_softcap_without_launch():
    """With USP_ATTN_SOFTCAP a cap that is not finite and > 0 is USP_EINVAL, and the 64-row family forced is
    USP_EUNSUPPORTED -- both before anything is launched (host memory stands in for the device pointers)."""
    _C, L = _lib()
    buf = ctypes.create_string_buffer(4096)
    addr = (ctypes.addressof(buf) + 15) & ~15
    for make, call in ((_valid_fwd, L.usp_flash_fwd), (_valid_bwd, L.usp_flash_bwd)):
        for bad in (-1.0, 0.0, float("nan"), float("inf"), float("-inf")):
            a = make(_C, addr)
            a.flags, a.softcap = _C.USP_ATTN_SOFTCAP, bad
            assert call(ctypes.byref(a), None) == -1, bad
        a = make(_C, addr)
        a.flags, a.softcap = _C.USP_ATTN_SOFTCAP | _C.USP_FORCE_ROW64, 30.0
        assert call(ctypes.byref(a), None) == -2
        a.softmax_scale = 0.0                              # the existing checks still come first
        assert call(ctypes.byref(a), None) == -1


# ---- Python surface: what is still refused, and a bad cap ------------------------------------------------------------------------------
def test_python_refusals_unchanged_and_bad_softcap_raises():
    import yunchang_amd as Y
    from yunchang_amd.kernels.attention import hip_attn_func, hip_attn_forward
    from yunchang_amd.kernels.features import Features

    def _check_plain(dropout_p, softcap, alibi_slopes):      # (no operands: the combination is judged before the slopes' shape)
        return Features.of(None, None, False, softcap=softcap, alibi_slopes=alibi_slopes, dropout_p=dropout_p).softcap
    from yunchang_amd.ring.zigzag_ring_flash_attn import _check_hot_path_args
    q = torch.zeros(1, 8, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        _check_plain(0.1, 30.0, None)                       # dropout
    with pytest.raises(NotImplementedError):
        _check_plain(0.0, 30.0, torch.ones(2))              # ALiBi
    with pytest.raises(NotImplementedError):
        hip_attn_forward(*(torch.zeros(1, 8, 2, 256, dtype=torch.bfloat16),) * 3, softcap=30.0)   # D = 256
    with pytest.raises(NotImplementedError):
        _check_hot_path_args(0.0, (4, 0), 30.0)             # a window across the ring
    with pytest.raises(NotImplementedError):
        _check_hot_path_args(0.1, (-1, -1), 30.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _check_plain(0.0, bad, None)
        with pytest.raises(ValueError):
            _check_hot_path_args(0.0, (-1, -1), bad)
        with pytest.raises(ValueError):
            hip_attn_func(q, q, q, softcap=bad)
    assert _check_plain(0.0, None, None) is None and _check_plain(0.0, 0, None) is None
    assert _check_plain(0.0, 30, None) == 30.0
    _check_hot_path_args(0.0, (-1, -1), 30.0)               # served now
    assert Y.LongContextAttention is not None


def test_softcap_keyword_reaches_the_backend_only_when_on():
    """Backends written before softcap (tests/oracle_backend.py) take no softcap keyword: a call without a cap must not
    pass one; a call with one passes it to every flash call."""
    from yunchang_amd.kernels import attention as A
    seen = []

    class Rec:
        def fwd(self, *a, **kw):
            seen.append(("fwd", kw.get("softcap")))

        def bwd(self, *a, **kw):
            seen.append(("bwd", kw.get("softcap")))

        def add(self, *a):
            seen.append(("add", None))
    prev = A.set_block_backend(Rec())
    try:
        for cap in (None, 0, 0.0):
            assert A.get_block_backend(softcap=cap) is A._BACKEND
        be = A.get_block_backend(softcap=7)
        be.fwd(1, 2)
        be.bwd(3)
        be.add(4)
    finally:
        A.set_block_backend(prev)
    assert seen == [("fwd", 7.0), ("bwd", 7.0), ("add", None)]


def test_reference_cap_bites_in_the_gloo_cases():
    """The distributed cases below use q x 4 and a cap of 3: softcap moves every reference quantity by > 10 x tolerance."""
    q, k, v, do = make_case(1, 64, 64, 4, 2, 32, seed=1)
    assert_cap_bites(np64(q), np64(k), np64(v), np64(do), 32 ** -0.5, 3.0, True, None, 2e-2, 5e-2)


# ---- a softcap-aware numpy block backend --------------------------------------------------------------------------------------------
def _softcap_backend():
    from oracle_backend import OracleBlockBackend, _np, _put
    from oracle import usp_oracle as O

    class SoftcapOracleBackend(OracleBlockBackend):
        """OracleBlockBackend with the `softcap` keyword of HipBlockBackend (the fp64 reference above)."""
        name = "oracle-softcap"
        _cap = None                      # packed calls: the cap of the sequence-by-sequence dense calls

        def fwd(self, q, k, v, softmax_scale, causal, lse, out=None, acc=None, merge_in=False,
                final_begin=0, final_end=None, window=None, k_splits=None, softcap=None):
            cap = softcap if softcap is not None else self._cap
            if cap is None:
                return super().fwd(q, k, v, softmax_scale, causal, lse, out, acc, merge_in, final_begin, final_end,
                                   window, k_splits)
            self.calls.append(("fwd-softcap", float(cap)))
            Sq = q.shape[1]
            fe = Sq if final_end is None else final_end
            bo, bl = ref_fwd(_np(q), _np(k), _np(v), softmax_scale, cap, causal, window)
            if merge_in:
                o_new, l_new = O.update_out_and_lse(_np(acc), np.swapaxes(_np(lse), 1, 2)[..., None], bo, bl)
                bo, bl = o_new, np.swapaxes(l_new[..., 0], 1, 2)
            _put(lse, bl)
            if fe > final_begin:
                _put(out[:, final_begin:fe], bo[:, final_begin:fe])
            if final_begin > 0:
                _put(acc[:, :final_begin], bo[:, :final_begin])
            if fe < Sq:
                _put(acc[:, fe:], bo[:, fe:])

        def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale, causal, accum_dq=False,
                accum_dk=False, accum_dv=False, dq16=None, dk16=None, dv16=None, window=None, only=None, softcap=None):
            cap = softcap if softcap is not None else self._cap
            if cap is None:
                return super().bwd(dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale, causal, accum_dq, accum_dk,
                                   accum_dv, dq16, dk16, dv16, window, only)
            self.calls.append(("bwd-softcap", float(cap)))
            grads = ref_bwd_from(_np(dout), _np(q), _np(k), _np(v), _np(lse), _np(delta), softmax_scale, cap, causal, window)
            wanted = {None: ("dq", "dk", "dv"), "dq": ("dq",), "dkdv": ("dk", "dv")}[only]
            for nm, dst, d16, val, accum in (("dq", dq, dq16, grads[0], accum_dq), ("dk", dk, dk16, grads[1], accum_dk),
                                             ("dv", dv, dv16, grads[2], accum_dv)):
                if nm in wanted:
                    _put(d16 if d16 is not None else dst, val + _np(dst) if accum else val)

        def fwd_packed(self, *a, softcap=None, **kw):
            self._cap = softcap
            try:
                return super().fwd_packed(*a, **kw)
            finally:
                self._cap = None

        def bwd_packed(self, *a, softcap=None, **kw):
            self._cap = softcap
            try:
                return super().bwd_packed(*a, **kw)
            finally:
                self._cap = None

    return SoftcapOracleBackend()


# ---- USP layer and rings on gloo ranks ---------------------------------------------------------------------------------------
CAP = 3.0


def _usp_worker(rank, ws, ud, rd, impl, causal, Hq, Hkv):
    """LongContextAttention (default, pipelined path) with softcap against the fp64 reference on the global tensors."""
    import yunchang_amd as Y
    import yunchang_amd.hybrid.async_attn_layer as AL
    from yunchang_amd.kernels import set_block_backend
    be = _softcap_backend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    AL._FILL_ITEMS = 1                  # tiny problem: let the head-group pipeline form anyway
    B, S, D = 1, 64, 32
    q, k, v, do = make_case(B, S, S, Hq, Hkv, D, seed=1)
    scale = D ** -0.5
    qn, kn, vn, don = (np64(t) for t in (q, k, v, do))
    ro, _ = ref_fwd(qn, kn, vn, scale, CAP, causal)
    ext = Y.EXTRACT_FUNC_DICT[impl]
    truth = [ext(torch.from_numpy(np.ascontiguousarray(t)), rank, world_size=ws, rd=rd, ud=ud).float()
             for t in (ro,) + tuple(ref_bwd(don, qn, kn, vn, scale, CAP, causal))]
    lq, lk, lv, ldo = (ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in (q, k, v, do))
    for t in (lq, lk, lv):
        t.requires_grad_(True)
    out = Y.LongContextAttention(ring_impl_type=impl)(lq, lk, lv, causal=causal, softcap=CAP)
    out.backward(ldo)
    got = [t.detach().float() for t in (out, lq.grad, lk.grad, lv.grad)]
    capped = {c[0] for c in be.calls}
    ok = all(torch.allclose(a, t, atol=tol, rtol=tol) for a, t, tol in zip(got, truth, (2e-2, 5e-2, 5e-2, 5e-2)))
    return ok, sorted(capped)


@pytest.mark.parametrize("ws,ud,rd,impl,causal,Hq,Hkv", [(4, 2, 2, "zigzag", True, 4, 2),
                                                         (4, 1, 4, "basic", False, 4, 4)])
def test_usp_layer_with_softcap_matches_reference(ws, ud, rd, impl, causal, Hq, Hkv):
    """Ulysses 2 x ring 2 (zigzag, causal, GQA) and ring 1 x 4 (basic, full): forward + backward equal the fp64 softcap
    reference, and every block launch carried the cap (only capped calls reached the backend)."""
    for ok, kinds in run_distributed(_usp_worker, ws, ud, rd, impl, causal, Hq, Hkv):
        assert ok
        assert kinds == ["bwd-softcap", "fwd-softcap"], kinds


def _varlen_worker(rank, ws, lens, Hq, Hkv):
    import torch.distributed as dist
    import yunchang_amd as Y
    from yunchang_amd.kernels import set_block_backend
    be = _softcap_backend()
    set_block_backend(be)
    D, T = 32, sum(lens)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    q, k, v, do = (t[0] for t in make_case(1, T, T, Hq, Hkv, D, seed=2))
    scale = D ** -0.5
    truth = [np.zeros((T, h, D)) for h in (Hq, Hq, Hkv, Hkv)]
    for a, b in zip(cu[:-1], cu[1:]):
        qn, kn, vn, don = (np64(t[a:b])[None] for t in (q, k, v, do))
        ro, _ = ref_fwd(qn, kn, vn, scale, CAP, True)
        for dst, val in zip(truth, (ro,) + tuple(ref_bwd(don, qn, kn, vn, scale, CAP, True))):
            dst[a:b] = val[0]
    truth = [Y.extract_local_varlen(torch.from_numpy(t), cu, rank, ws, "zigzag").float() for t in truth]
    lq, lk, lv, ldo = (Y.extract_local_varlen(t, cu, rank, ws, "zigzag") for t in (q, k, v, do))
    for t in (lq, lk, lv):
        t.requires_grad_(True)
    out = Y.zigzag_ring_flash_attn_varlen_func(lq, lk, lv, torch.tensor(cu // ws, dtype=torch.int32), int(max(lens)) // ws,
                                               causal=True, softcap=CAP, group=dist.group.WORLD)
    out.backward(ldo)
    got = [t.detach().float() for t in (out, lq.grad, lk.grad, lv.grad)]
    return all(torch.allclose(a, t, atol=tol, rtol=tol) for a, t, tol in zip(got, truth, (2e-2, 5e-2, 5e-2, 5e-2))) and \
        {c[0] for c in be.calls} == {"fwd-softcap", "bwd-softcap"}


def test_zigzag_varlen_ring_with_softcap_matches_reference():
    """The packed zigzag ring at degree 2, GQA, three sequences: forward + backward with softcap."""
    assert all(run_distributed(_varlen_worker, 2, (32, 64, 16), 4, 2))
