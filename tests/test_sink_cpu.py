"""Attention sinks (sinks) without a GPU: the fp64 reference against torch autograd of the written-out formula, mutant references
against the gates the GPU tests use, what the C ABI refuses before any launch (usp_flash_fwd_sink / usp_sink_bwd), the Python
refusals and the validation of the tensor, and the schedules -- the basic, zigzag and stripe rings, Ulysses head slices, 2-D grids,
the global window beside them -- on gloo ranks with a sink-aware oracle backend, against the unsharded fp64 reference."""
import ctypes
import os
import re

import pytest
import torch

import sink_ref
from dist_util import run_distributed
from golden_util import TOL, assert_close, grad_tol
from sink_ref import SinkOracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINKS4 = (-30.0, 0.0, 3.0, 12.0)          # no effect | off-by-one softmax | a strong sink | above every score


def _draw(B, Sq, Sk, Hq, Hkv, D, seed, dtype=torch.float64):
    """q, k ~ N(0, 1); v, dout ~ N(1, 1): the delta_i = dout_i . out_i then do not cancel in ds_h."""
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(B, s, h, D, generator=g, dtype=torch.float64) for s, h in ((Sq, Hq), (Sk, Hkv), (Sk, Hkv), (Sq, Hq)))
    return [t.to(dtype) for t in (q, k, v + 1.0, do + 1.0)]


# ---- 1. the reference against autograd of the written-out formula -------------------------------------------------------------
@pytest.mark.parametrize("Sq,Sk,causal,window,shift", [(24, 40, True, None, 0), (40, 24, True, None, 0), (32, 32, False, (9, 4), 0),
                                                       (24, 40, True, (12, 0), 7), (24, 40, False, None, 0), (16, 48, True, (5, 0), -40)])
def test_reference_against_autograd(Sq, Sk, causal, window, shift):
    """A sink column appended to the scores, softmax, the column dropped; (40, 24) causal and the shifted window have rows that
    see no key: the column keeps their softmax finite (lse = s_h, out = 0)."""
    B, Hq, Hkv, D = 2, 4, 2, 16
    q, k, v, do = _draw(B, Sq, Sk, Hq, Hkv, D, 3)
    sinks = torch.tensor(SINKS4, dtype=torch.float64)
    scale = 0.3
    out, lse, dq, dk, dv, ds = sink_ref.ref_bwd(do, q, k, v, scale, sinks, causal, window, shift)
    ql, kl, vl, sl = (t.clone().requires_grad_(True) for t in (q, k, v, sinks))
    vis = sink_ref.alibi_ref.visible(Sq, Sk, causal, window, shift)
    empty = ~vis.any(1)
    assert bool(empty.any()) == ((Sq, Sk) == (40, 24) or shift == -40)
    outs, lses = [], []
    for b in range(B):
        per_head = []
        for h in range(Hq):
            s = (scale * ql[b, :, h] @ kl[b, :, h // (Hq // Hkv)].T).masked_fill(~vis, float("-inf"))
            s1 = torch.cat([s, sl[h].expand(Sq, 1)], dim=1)                 # NOT multiplied by the scale
            per_head.append(torch.softmax(s1, -1)[:, :Sk] @ vl[b, :, h // (Hq // Hkv)])
            lses.append(torch.logsumexp(s1, -1))
        outs.append(torch.stack(per_head, 1))
    o2 = torch.stack(outs)
    o2.backward(do)
    assert torch.allclose(out, o2.detach(), atol=1e-12, rtol=1e-10)
    l2 = torch.stack(lses).detach().reshape(B, Hq, Sq)
    assert torch.allclose(lse, l2, atol=1e-12, rtol=1e-10)
    for got, want in ((dq, ql.grad), (dk, kl.grad), (dv, vl.grad), (ds, sl.grad)):
        assert torch.allclose(got, want, atol=1e-11, rtol=1e-9)
    if bool(empty.any()):                                                   # never -inf: an empty row holds the sink alone
        assert torch.equal(lse[:, :, empty], sinks[None, :, None].expand(B, Hq, int(empty.sum())))
        assert not out[:, empty].any() and bool(torch.isfinite(lse).all())
    # sinks = None is the plain function
    o0, l0 = sink_ref.ref_fwd(q, k, v, scale, None, causal, window, shift)
    o1, l1 = sink_ref.alibi_ref.ref_fwd(q, k, v, scale, None, causal, window, shift)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    assert sink_ref.ref_bwd_from(do, q, k, v, o0, l0, scale, None, causal, window, shift)[3] is None


def test_mutant_references_are_far_away():
    """What a WRONG sink costs against the gates of tests/test_gpu_sink.py (out / dq / dk / dv at golden_util.TOL, dsinks at
    rtol x sum |terms|): every mutant misses them by a wide margin -- 5 x the gate at the least."""
    B, S, Hq, Hkv, D = 2, 96, 4, 2, 32
    q, k, v, do = _draw(B, S, S, Hq, Hkv, D, 5)
    sinks = torch.tensor(SINKS4, dtype=torch.float64)
    scale = D ** -0.5
    truth = sink_ref.ref_bwd(do, q, k, v, scale, sinks, True)
    atol, rtol = TOL["bfloat16"]["out"]

    def excess(got, want, a, r):                                            # largest error in units of its gate
        return float(((got - want).abs() / (a + r * want.abs())).max())

    ln2 = torch.log(torch.tensor(2.0, dtype=torch.float64))
    dropped = sinks.clone()
    dropped[2] = -1e30                                                      # (the head whose sink is 3)
    for name, m in (("counted twice", sinks + ln2), ("multiplied by the scale", sinks * scale), ("dropped on one head", dropped)):
        got = sink_ref.ref_bwd(do, q, k, v, scale, m, True)
        assert excess(got[0], truth[0], atol, rtol) > 5, name              # out
        assert excess(got[1], truth[1], atol, rtol) > 5, name              # lse (gated like out, as the ALiBi tests do)
        assert max(excess(g, w, *TOL["bfloat16"]["grad"]) for g, w in zip(got[2:5], truth[2:5])) > 5, name
    delta = (do * truth[0]).sum(-1).transpose(1, 2)
    terms = sink_ref.sink_terms(sinks, truth[1], delta)
    gate = TOL["bfloat16"]["grad"][1] * terms.abs().sum(dim=(0, 2))
    assert bool((truth[5].abs() >= 0.5 * terms.abs().sum(dim=(0, 2))).all()), "the deltas must not cancel"
    live = torch.tensor([False, True, True, True])                          # (head 0: exp(-30 - lse) is nothing in fp64 either)
    for name, bad in (("wrong sign", -truth[5]), ("one batch missing", -terms[1:].sum(dim=(0, 2)))):
        assert bool((((bad - truth[5]).abs() > 5 * gate) | ~live).all()), name


# ---- 2. the C ABI at the host ---------------------------------------------------------------------------------------------------
def _lib():
    from yunchang_amd import _C
    if not os.path.exists(_C.lib_path()):
        pytest.fail("libusp_hip.so is not built: run __graft_entry__.build() first")
    return _C, _C.load()


def _args(_C, addr):
    a = _C.UspFwdArgs()
    a.dtype, a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D = 0, 1, 16, 16, 2, 2, 128
    a.softmax_scale = 0.125
    a.lse = addr
    a.q.ptr = a.k.ptr = a.v.ptr = a.out.ptr = a.acc.ptr = addr
    a.final_end = a.Sq
    for t in (a.q, a.k, a.v, a.out, a.acc):
        t.stride_b, t.stride_s, t.stride_h = 16 * 2 * 128, 2 * 128, 128
    return a


def test_abi_feature_bit_entry_points_and_unchanged_structs():
    _C, L = _lib()
    txt = open(os.path.join(ROOT, "include", "usp_hip.h")).read()
    assert _C.USP_ATTN_SINK == 1024 == int(re.search(r"#define USP_ATTN_SINK (\d+)", txt).group(1))
    assert L.usp_attn_features() & _C.USP_ATTN_SINK
    assert L.usp_attn_features() & (2 | 64 | 128 | 256 | 512) == 2 | 64 | 128 | 256 | 512
    assert L.usp_abi_version() == 7 == _C.ABI_VERSION
    for name in ("usp_flash_fwd_sink", "usp_sink_bwd"):
        assert name in _C.SINK_EXPORTS and name in _C.EXPORTS and hasattr(L, name)
        assert _C._sink_entry(name).restype is ctypes.c_int
    assert _C._sink_entry("usp_flash_fwd_sink").argtypes[1:] == [ctypes.c_void_p, ctypes.c_void_p]
    assert len(_C._sink_entry("usp_sink_bwd").argtypes) == 13
    assert re.search(r"int usp_flash_fwd_sink\(const usp_fwd_args\* args, const float\* sinks, void\* stream\);", txt)
    assert re.search(r"int usp_sink_bwd\(int32_t B, int32_t S, int32_t H, const float\* sinks, const float\* lse, int64_t lse_stride_b,\s+"
                     r"int64_t lse_stride_h, const float\* delta, int64_t delta_stride_b, int64_t delta_stride_h, float\* dsinks,\s+"
                     r"int32_t accum, void\* stream\);", txt)
    assert not hasattr(L, "usp_flash_bwd_sink")                 # usp_flash_bwd with the sink-including lse IS the backward
    for cls in (_C.UspFwdArgs, _C.UspBwdArgs):
        assert cls._fields_[-1] == ("softcap", ctypes.c_float)
    assert len(re.findall(r"typedef struct", txt)) == 3
    assert ctypes.sizeof(_C.UspFwdArgs) == 296 and ctypes.sizeof(_C.UspBwdArgs) == 504 and ctypes.sizeof(_C.UspTensor) == 32


def test_abi_declines_without_launch():
    """Host memory stands in for the device pointers (the sinks included): every call below returns before anything is launched."""
    _C, L = _lib()
    fwd, sbwd = _C._sink_entry("usp_flash_fwd_sink"), _C._sink_entry("usp_sink_bwd")
    buf = ctypes.create_string_buffer(1 << 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    seq = (ctypes.c_int32 * 2)(0, 16)
    sinks = (ctypes.c_float * 2)(0.5, 0.25)
    sp = ctypes.cast(sinks, ctypes.c_void_p)
    a = _args(_C, addr)                            # the sink belongs to the launch that opens the rows' state
    a.merge_in = 1
    assert fwd(ctypes.byref(a), sp, None) == -1
    a = _args(_C, addr)                            # softcap together with sinks
    a.flags, a.softcap = _C.USP_ATTN_SOFTCAP, 30.0
    assert fwd(ctypes.byref(a), sp, None) == -2
    a = _args(_C, addr)                            # a packed batch
    a.seq_q = a.seq_k = ctypes.addressof(seq)
    assert fwd(ctypes.byref(a), sp, None) == -2
    a = _args(_C, addr)                            # the 64-row family forced
    a.flags = _C.USP_FORCE_ROW64
    assert fwd(ctypes.byref(a), sp, None) == -2
    a = _args(_C, addr)                            # the existing checks still come first
    a.flags, a.softmax_scale = _C.USP_FORCE_ROW64, 0.0
    assert fwd(ctypes.byref(a), sp, None) == -1
    a = _args(_C, addr)
    a.flags = _C.USP_FORCE_ROW64 | _C.USP_FORCE_WAVE32
    assert fwd(ctypes.byref(a), sp, None) == -1
    a = _args(_C, addr)
    a.flags, a.D = _C.USP_FORCE_ROW64, 96
    assert fwd(ctypes.byref(a), sp, None) == -2
    # sinks = NULL is usp_flash_fwd: the plain path's own checks answer, merge_in and softcap are no longer refused as such
    a = _args(_C, addr)
    a.merge_in, a.acc.ptr = 1, None
    assert fwd(ctypes.byref(a), None, None) == L.usp_flash_fwd(ctypes.byref(a), None) == -1      # (merge_in needs acc)
    a = _args(_C, addr)
    a.flags, a.D = _C.USP_FORCE_ROW64, 64
    assert fwd(ctypes.byref(a), None, None) == L.usp_flash_fwd(ctypes.byref(a), None) == -2      # (the family's own refusal)
    assert L.usp_last_launch_kinds() == 0
    # usp_sink_bwd: null pointers and non-positive sizes
    for bad in ((0, 4, 2, sp, addr, addr, addr), (1, 0, 2, sp, addr, addr, addr), (1, 4, 0, sp, addr, addr, addr),
                (1, 4, 2, None, addr, addr, addr), (1, 4, 2, sp, None, addr, addr), (1, 4, 2, sp, addr, None, addr),
                (1, 4, 2, sp, addr, addr, None)):
        B, S, H, s, l, d, o = bad
        assert sbwd(B, S, H, s, l, 8, 4, d, 8, 4, o, 0, None) == -1, bad


# ---- 3. Python: validation and refusals -----------------------------------------------------------------------------------------
def test_sinks_value_shape_dtype_device():
    from yunchang_amd import _C
    cpu = torch.device("cpu")
    assert _C.sinks_value(None, 4, cpu) is None
    for good in (torch.rand(4), torch.rand(4).to(torch.bfloat16), torch.rand(4).to(torch.float16), torch.rand(8)[::2],
                 torch.rand(4, requires_grad=True)):
        t = _C.sinks_value(good, 4, cpu)
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (4,) and not t.requires_grad
        assert torch.equal(t, good.detach().float())
    assert _C.sinks_value(torch.rand(4).to(torch.bfloat16), 4, cpu, torch.bfloat16) is not None
    for bad in (torch.rand(3), torch.rand(1, 4), torch.rand(4, 1), torch.rand(4).double(), torch.rand(4).to("meta"), [0.5] * 4, 0.5):
        with pytest.raises(ValueError):
            _C.sinks_value(bad, 4, cpu)
    with pytest.raises(ValueError):                 # the OTHER 16-bit type than the operands'
        _C.sinks_value(torch.rand(4).to(torch.float16), 4, cpu, torch.bfloat16)


def test_python_refusals(monkeypatch):
    import yunchang_amd as Y
    from yunchang_amd import _C
    from yunchang_amd.comm.all_to_all import local_sinks
    from yunchang_amd.kernels import attention as KA
    from yunchang_amd.ring import block_pieces
    from yunchang_amd.ring.ring_flash_attn_varlen import ring_flash_attn_varlen_func
    from yunchang_amd.ring.zigzag_ring_flash_attn_varlen import zigzag_ring_flash_attn_varlen_func
    q = torch.zeros(2, 16, 4, 64, dtype=torch.bfloat16)
    s = torch.tensor(SINKS4)
    m = torch.rand(4)
    # sinks together with a second score-level step: no kernel holds both
    for kw, what in ((dict(softcap=30.0), "softcap"), (dict(alibi_slopes=m), "alibi_slopes"), (dict(dropout_p=0.1), "dropout_p")):
        for call in (lambda: KA.hip_attn_func(q, q, q, sinks=s, **kw), lambda: KA.hip_attn_forward(q, q, q, sinks=s, **kw),
                     lambda: KA.hip_attn_backward(q, q, q, q, q, None, q, q, q, sinks=s, dsinks=torch.zeros(4), **kw),
                     lambda: Y.ring_flash_attn_func(q, q, q, causal=True, sinks=s, **kw),
                     lambda: Y.zigzag_ring_flash_attn_func(q, q, q, causal=True, sinks=s, **kw),
                     lambda: Y.stripe_flash_attn_func(q, q, q, causal=True, sinks=s, **kw)):
            with pytest.raises(NotImplementedError, match="sinks together with " + what):
                call()
    for kw in (dict(softcap=30.0), dict(alibi=m), dict(dropout=(0.1, 1, 0))):
        with pytest.raises(NotImplementedError, match="sinks together with"):
            KA.get_block_backend(sinks=s, **kw)
    with pytest.raises(ValueError, match="dsinks"):
        KA.hip_attn_backward(q, q, q, q, q, None, q, q, q, sinks=s)
    # shape, dtype and device are ValueErrors before anything touches a device
    for bad in (torch.rand(5), torch.rand(4).double(), torch.rand(4).to(torch.float16), torch.rand(4).to("meta")):
        for call in (lambda: KA.hip_attn_forward(q, q, q, sinks=bad), lambda: KA.hip_attn_func(q, q, q, sinks=bad),
                     lambda: Y.ring_flash_attn_func(q, q, q, causal=True, sinks=bad)):
            with pytest.raises(ValueError):
                call()
    # the wrapper: only launches without merge_in carry the sinks; packed ones refuse; older backends are untouched without sinks
    seen = []

    class Rec:
        def fwd(self, *a, **kw):
            seen.append(kw)

        def bwd(self, *a, **kw):
            seen.append(("bwd", kw))

        def sink_grad(self, sinks, lse, delta, out=None, accum=False):
            return ("grad", sinks, lse, delta, out, accum)

        def merge(self):
            return "merge"
    prev = KA.set_block_backend(Rec())
    try:
        be = KA.get_block_backend(sinks=s)
        be.fwd(0, 1, 2, 3, 4, 5, 6, 7, False, window=(3, 0))
        be.fwd(0, 1, 2, 3, 4, 5, 6, 7, True, 0, 9)
        be.fwd(0, 1, 2, 3, 4, 5, merge_in=True)
        be.fwd(0, 1, 2, 3, 4, 5)
        be.bwd(2)
        assert seen == [{"sinks": s, "window": (3, 0)}, {}, {"merge_in": True}, {"sinks": s}, ("bwd", {})]
        assert be.sink_grad("l", "d", out="o") == ("grad", s, "l", "d", "o", False) and be.merge() == "merge"
        for packed in (be.fwd_packed, be.bwd_packed):
            with pytest.raises(NotImplementedError, match="packed"):
                packed()
        assert isinstance(KA.get_block_backend(), Rec) and isinstance(KA.get_block_backend(sinks=None), Rec)
    finally:
        KA.set_block_backend(prev)
    # the packed rings refuse and say what serves it; so do the pieces and the async layer, which name LongContextAttention
    t3 = torch.zeros(32, 4, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 32], dtype=torch.int32)
    for f in (ring_flash_attn_varlen_func, zigzag_ring_flash_attn_varlen_func):
        with pytest.raises(NotImplementedError, match="packed"):
            f(t3, t3, t3, cu, 32, causal=True, sinks=s)
    with pytest.raises(NotImplementedError, match="LongContextAttention"):
        block_pieces.refuse_sinks(s, True)
    block_pieces.refuse_sinks(s, False)
    block_pieces.refuse_sinks(None, True)
    # the sinks cut by the head map of the exchange: a slice, so autograd scatters the gradient back
    s8 = torch.arange(8.0, requires_grad=True)
    cut = local_sinks(s8, 8, 4, 1)
    assert torch.equal(cut.detach(), torch.tensor([2.0, 3.0]))
    cut.sum().backward()
    assert torch.equal(s8.grad, torch.tensor([0, 0, 1.0, 1.0, 0, 0, 0, 0]))
    loc = torch.rand(2)
    assert local_sinks(loc, 8, 4, 1) is loc and local_sinks(None, 8, 4, 1) is None and local_sinks(s8, 8, 1, 0) is s8
    for bad in (torch.rand(3), torch.rand(2, 8)):
        with pytest.raises(ValueError):
            local_sinks(bad, 8, 4, 1)

    # a library without the feature bit
    class Old:
        @staticmethod
        def usp_attn_features():
            return 2 | 64 | 128 | 256 | 512
    monkeypatch.setattr(_C, "load", lambda: Old)
    with pytest.raises(NotImplementedError, match="rebuild it"):
        _C._sink_entry("usp_flash_fwd_sink")


# ---- 4. the schedules on gloo ---------------------------------------------------------------------------------------------------
B, H, D, CH = 2, 4, 32, 32                # CH rows per rank (even: the zigzag layout)
SCALE = D ** -0.5
IMPLS = ("basic", "zigzag", "strip")


def _inputs(ws, hkv):
    q, k, v, do = _draw(B, CH * ws, CH * ws, H, hkv, D, 11 + hkv)
    return [t.to(torch.bfloat16) for t in (q, k, v, do)]


_TRUTH = {}


def _truth(ws, hkv, causal=True, window=None):
    """(out, dq, dk, dv, dsinks, sum |terms|) of the unsharded problem, computed once per case."""
    key = (ws, hkv, causal, window)
    if key not in _TRUTH:
        q, k, v, do = _inputs(ws, hkv)
        sinks = torch.tensor(SINKS4)
        r = sink_ref.ref_bwd(do, q, k, v, SCALE, sinks, causal, window, 0, out_dtype=torch.bfloat16)
        delta = (do.double() * r[0].to(torch.bfloat16).double()).sum(-1).transpose(1, 2)
        _TRUTH[key] = (r[0],) + r[2:] + (sink_ref.sink_terms(sinks, r[1], delta).abs().sum(dim=(0, 2)),)
    return _TRUTH[key]


def _covered_once(log, rows):
    """Every row of the rank opened by exactly one sink-carrying launch; no merge_in launch carries one."""
    count = [0] * rows
    for row0, n, has_sink, merge_in in log:
        assert has_sink != merge_in, (row0, n, has_sink, merge_in)
        if has_sink:
            for i in range(row0, row0 + n):
                count[i] += 1
    return count == [1] * rows


def _rows(ext, rank, ws, ud, rd):
    """The rows of the whole sequence this rank holds under `ext`'s layout (the extract functions ask torch.distributed for the
    grid, so the ranks do it and the parent cuts the truth by the answer)."""
    idx = torch.arange(CH * ws, dtype=torch.float32)[None, :, None, None]
    return ext(idx, rank, world_size=ws, rd=rd, ud=ud).flatten().long().tolist()


def _run(layer_call, loc, sinks_full, be):
    """One forward + backward on this rank -> [out, dq, dk, dv] (numpy), the ALL-REDUCED dsinks, the launch log's verdict."""
    import torch.distributed as dist
    del be.sink_log[:]
    ts = [t.detach().clone().requires_grad_(True) for t in loc[:-1]]
    s = sinks_full.clone().requires_grad_(True)
    out = layer_call(*ts, s)
    fwd_log = list(be.sink_log)
    out.backward(loc[-1])
    assert s.grad.dtype == s.dtype and s.grad.shape == s.shape
    share = s.grad.detach().clone()
    total = share.float().clone()
    dist.all_reduce(total)                                  # the gradient contract: the SUM over the group; the layers do none
    return [t.detach().float().numpy() for t in [out] + [t.grad for t in ts]], total.numpy(), share.float().numpy(), fwd_log


def _grid_worker(rank, ws, ud, rd):
    import yunchang_amd as Y
    from yunchang_amd.kernels import set_block_backend
    be = SinkOracleBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    os.environ.pop("USP_RING_WINDOW", None)
    sinks = torch.tensor(SINKS4)
    res = {}
    for impl in IMPLS:
        ext = Y.EXTRACT_FUNC_DICT[impl]
        res[(impl, "rows")] = _rows(ext, rank, ws, ud, rd)
        loc = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in _inputs(ws, 2)]
        attn = Y.LongContextAttention(ring_impl_type=impl)
        got = _run(lambda q, k, v, s: attn(q, k, v, causal=True, sinks=s), loc, sinks, be)
        res[(impl, "layer")] = got[:3] + (_covered_once(got[3], CH * ws // rd),)
        # the QKV-packed layer (equal head counts), the sinks in the operands' 16-bit type
        lq, lk, lv, ldo = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in _inputs(ws, H)]
        packed = Y.LongContextAttentionQKVPacked(ring_impl_type=impl)
        got = _run(lambda qkv, s: packed(qkv, causal=True, sinks=s), [torch.stack([lq, lk, lv], dim=2), ldo],
                   sinks.to(torch.bfloat16), be)
        g = got[0][1]                                        # d(qkv): (B, S, 3, H, D)
        res[(impl, "packed")] = ([got[0][0], g[:, :, 0], g[:, :, 1], g[:, :, 2]],) + got[1:3] + (_covered_once(got[3], CH * ws // rd),)
    # the async layer refuses and names the layer that serves it
    try:
        Y.AsyncLongContextAttention(ring_impl_type="basic")(*loc[:3], causal=True, sinks=sinks)
        res["async"] = False
    except NotImplementedError as e:
        res["async"] = "LongContextAttention" in str(e)
    return res


def _check_rank(got, truth, rows, rank, ws, what, sinks_dtype_bf16=False):
    arrays, total, share, once = got
    assert once, f"{what}: a row range was opened by more or fewer than one sink-carrying launch"
    for g, w, name in zip(arrays, truth[:4], ("out", "dq", "dk", "dv")):
        w = w[:, rows]
        tol = TOL["bfloat16"]["out"] if name == "out" else grad_tol("bfloat16", 2)
        assert_close(g, w, *tol, f"{what} rank {rank} {name}")
    ds, sum_terms = truth[4].numpy(), truth[5].numpy()
    # the all-reduced gradient is the single-device one: rtol of the gradients x sum |terms| (+ bf16 rounding of a 16-bit grad)
    gate = TOL["bfloat16"]["grad"][1] * sum_terms + (2.0 ** -7 * abs(ds) * ws if sinks_dtype_bf16 else 0.0)
    assert (abs(total - ds) <= gate).all(), (what, rank, total, ds, gate)
    return share


@pytest.mark.parametrize("ws,ud,rd", [(2, 1, 2), (4, 1, 4), (4, 2, 2), (4, 4, 1)])
def test_rings_and_layers_on_gloo(ws, ud, rd):
    from yunchang_amd.comm.all_to_all import local_heads
    res = run_distributed(_grid_worker, ws, ud, rd)
    for impl in IMPLS:
        for kind, hkv in (("layer", 2), ("packed", H)):
            for rank in range(ws):
                share = _check_rank(res[rank][(impl, kind)], _truth(ws, hkv), res[rank][(impl, "rows")], rank, ws,
                                    f"{impl} {kind} {ud}x{rd}", kind == "packed")
                hs = local_heads(H, ud, rank % ud)           # under Ulysses: the rank's heads, zeros elsewhere
                mask = torch.zeros(H, dtype=torch.bool)
                mask[hs] = True
                assert not share[~mask.numpy()].any(), (impl, kind, rank, share)
    assert all(r["async"] is True for r in res)


def _ulysses_worker(rank, ws):
    import torch.distributed as dist
    import yunchang_amd as Y
    from yunchang_amd.comm.all_to_all import local_heads
    from yunchang_amd.kernels import set_block_backend
    be = SinkOracleBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ws, 1, rank, ws)
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    loc = [ext(t, rank, world_size=ws, rd=1, ud=ws).detach().clone() for t in _inputs(ws, 2)]
    layer = Y.UlyssesAttention(dist.group.WORLD, attn_type=Y.AttnType.HIP)
    sinks = torch.tensor(SINKS4)
    res = {"rows": _rows(ext, rank, ws, ws, 1)}
    for name, s in (("full", sinks), ("local", sinks[local_heads(H, ws, rank)].clone())):
        got = _run(lambda q, k, v, st: layer(q, k, v, causal=True, sinks=st), loc, s, be)
        res[name] = got[:3] + (_covered_once(got[3], CH * ws),)
    try:
        layer(*loc[:3], causal=True, sinks=torch.rand(3))
        res["bad"] = False
    except ValueError:
        res["bad"] = True
    return res


def test_ulysses_slices_the_sinks():
    from yunchang_amd.comm.all_to_all import local_heads
    ws = 2
    res = run_distributed(_ulysses_worker, ws)
    truth = _truth(ws, 2)
    for rank in range(ws):
        rows = res[rank]["rows"]
        _check_rank(res[rank]["full"], truth, rows, rank, ws, "ulysses full")
        arrays, total, share, once = res[rank]["local"]      # sinks over the local heads: the gradient is the local heads' too
        assert once
        assert_close(arrays[0], truth[0][:, rows], *TOL["bfloat16"]["out"], "ulysses local out")
        hs = local_heads(H, ws, rank)
        assert (abs(share - truth[4].numpy()[hs]) <= TOL["bfloat16"]["grad"][1] * truth[5].numpy()[hs]).all()
        assert res[rank]["bad"] is True


def _window_worker(rank, ws):
    import yunchang_amd as Y
    from test_ring_window_cpu import ShiftOracleBackend
    from yunchang_amd.kernels import set_block_backend

    class Backend(SinkOracleBackend, ShiftOracleBackend):
        pass
    be = Backend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(1, ws, rank, ws)
    os.environ["USP_RING_WINDOW"] = "global"
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    loc = [ext(t, rank, world_size=ws, rd=ws, ud=1).detach().clone() for t in _inputs(ws, 2)]
    attn = Y.LongContextAttention(ring_impl_type="basic")
    got = _run(lambda q, k, v, s: attn(q, k, v, causal=True, window_size=WINDOW, sinks=s), loc, torch.tensor(SINKS4), be)
    shifts = [x[3] for x in be.launches if x[0] == "fwd"]
    return got[:3] + (_covered_once(got[3], CH),), shifts, _rows(ext, rank, ws, 1, ws)


WINDOW = (40, 0)


def test_windowed_basic_ring_with_the_global_window():
    """USP_RING_WINDOW=global beside sinks: the planner's first block opens the rows and carries the sink, the shifted ones merge."""
    ws = 4
    res = run_distributed(_window_worker, ws)
    truth = _truth(ws, 2, True, WINDOW)
    for rank in range(ws):
        _check_rank(res[rank][0], truth, res[rank][2], rank, ws, "windowed basic ring")
    assert any(s is not None and s > 0 for r in res for s in r[1]), "no shifted block was launched: the case is not the planner's"
