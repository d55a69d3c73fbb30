"""Bidirectional spans (bidirectional=) on the GPU: the span instantiations of the two-waves-per-SIMD kernels (usp_flash_fwd_span /
usp_flash_bwd_span) against tests/span_ref.py (fp64, on the device, the mask from the global definition alone) on needle inputs on
which one span end or start moved by one key or row is an O(1) error (tests/test_span_cpu.py::test_span_mutants_fail shows that
with the reference alone); off- and above-diagonal ring blocks; bit-identity with the document entry points; launch kinds and
refusals; strided layouts; hip_attn_func and LongContextAttention at a padded head dim; the basic ring on virtual ranks with a span
across a shard boundary; a small seeded fuzz.

Shapes: Sq = Sk in {320, 1280} -- 320 is ragged against the 128-key dK/dV block and the 128 / 256-row items, 1280 is several of
each -- with span ends on, one before and one after multiples of 64, spans of length 1 (a no-op), 2 and 3, one span of 700
(interior tiles take the pipelined loop, both ends are masked), one across row 256 and one ending at S.
Tolerances: the project's own (golden_util.TOL, grad_tol) and the lse bound of tests/test_gpu_doc_mask.py."""
import ctypes

import numpy as np
import pytest
import torch

import needle_inputs
import span_ref
from golden_util import TOL, assert_close, grad_tol

pytestmark = pytest.mark.gpu

SPANS = {320: [(5, 6), (62, 64), (64, 67), (127, 129), (190, 193), (250, 262), (300, 320)],
         1280: [(5, 6), (63, 65), (65, 68), (126, 128), (129, 131), (250, 262), (300, 1000), (1023, 1026), (1270, 1280)]}
CU_AROUND = {320: [0, 64, 200, 320], 1280: [0, 65, 300, 1100, 1280]}          # every span of SPANS inside one document
CU_DOCS = {320: [0, 63, 64, 65, 96, 128, 255, 256, 257, 320],                  # bidirectional="documents"
           1280: [0, 63, 64, 65, 96, 128, 255, 256, 257, 300, 1010, 1280]}
_WAVE_FWD = {"fwd_wave8", "fwd_wave4"}
_WAVE_BWD = {"dkdv_wave8", "dq_wave8", "reduce_heads"}


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _kind(kind, S):
    """(cu_doclens | None, bidirectional, the spans as pairs) of a parity case."""
    if kind == "alone":
        return None, SPANS[S], SPANS[S]
    if kind == "in-docs":
        return CU_AROUND[S], SPANS[S], SPANS[S]
    cu = CU_DOCS[S]
    return cu, "documents", list(zip(cu[:-1], cu[1:]))


def _arrays(dev, cu, bidirectional, row0, n_rows, key0, n_keys, S_total):
    from yunchang_amd.ring import doc_blocks
    plan = doc_blocks.parse_plan(cu, bidirectional, 1, S_total)
    host = doc_blocks.span_block_arrays(plan[0], plan.spans[0], row0, n_rows, key0, n_keys)
    return tuple(torch.from_numpy(a).to(dev) for a in host), host


_IN, _REF = {}, {}


def _inputs(dev, S, Hq, Hkv, D, dt, kind):
    key = (S, Hq, Hkv, D, dt, kind)
    if key not in _IN:
        cu, _, pairs = _kind(kind, S)
        nd = needle_inputs.make(S, S, Hq, Hkv, D, dt, C=8, seed=S + D, edges=span_ref.needle_edges(pairs, S, cu))
        _IN[key] = [torch.from_numpy(x.astype(np.float32)).to(getattr(torch, dt)).to(dev) for x in (nd.q, nd.k, nd.v, nd.do)]
    return _IN[key]


def _reference(key, do, q, k, v, scale, mask):
    if key not in _REF:
        _REF[key] = span_ref.ref_bwd(do, q, k, v, scale, mask, out_dtype=q.dtype)
    return _REF[key]


def _fwd(q, k, v, scale, causal, **kw):
    from yunchang_amd import _C
    out = torch.full_like(q, float("nan"))
    lse = torch.full((q.shape[0], q.shape[2], q.shape[1]), float("nan"), dtype=torch.float32, device=q.device)
    _C.flash_fwd(q, k, v, scale, causal, lse, out=out, **kw)
    return out, lse, _C.last_launch_kinds()


def _bwd(do, q, k, v, ref, scale, causal, **kw):
    from yunchang_amd import _C
    lse = ref[1].to(torch.float32)
    delta = torch.empty_like(lse)
    _C.bwd_delta(do, ref[0].to(q.dtype), delta)
    dq, dk, dv = (torch.full(t.shape, float("nan"), dtype=torch.float32, device=q.device) for t in (q, k, v))
    _C.flash_bwd(do, q, k, v, lse, delta, dq, dk, dv, scale, causal, **kw)
    return (dq, dk, dv), _C.last_launch_kinds()


def _check(out, lse, grads, ref, dt, G, what):
    assert_close(out, ref[0], *TOL[dt]["out"], f"{what} out")
    assert_close(lse, ref[1], 2e-3, 1e-4, f"{what} lse")
    for g, r, name in zip(grads, ref[2:], ("dq", "dk", "dv")):
        assert_close(g, r, *grad_tol(dt, G), f"{what} {name}")


# ---- 1. kernel parity ---------------------------------------------------------------------------------------------------------
PARITY = [(dt, D, 4, 1, 0, S, "alone") for dt in ("bfloat16", "float16") for D in (32, 64, 128) for S in (320, 1280)] + \
         [("bfloat16", 64, 4, 4, 0, 320, "alone"), ("float16", 128, 4, 4, 0, 1280, "alone"),
          ("bfloat16", 128, 4, 1, 1, 320, "alone"), ("float16", 64, 4, 1, 1, 1280, "alone"),
          ("bfloat16", 128, 4, 1, 0, 1280, "in-docs"), ("float16", 32, 4, 4, 1, 320, "in-docs"), ("bfloat16", 64, 4, 1, 0, 320, "in-docs"),
          ("float16", 128, 4, 1, 0, 320, "documents"), ("bfloat16", 64, 4, 4, 0, 1280, "documents"), ("bfloat16", 32, 4, 1, 1, 1280, "documents")]


@pytest.mark.parametrize("dt,D,Hq,Hkv,dkdv_heads,S,kind", PARITY, ids=lambda v: str(v))
def test_kernel_parity(dev, dt, D, Hq, Hkv, dkdv_heads, S, kind):
    cu, bidir, pairs = _kind(kind, S)
    q, k, v, do = _inputs(dev, S, Hq, Hkv, D, dt, kind)
    scale = D ** -0.5
    span, host = _arrays(dev, cu, bidir, 0, S, 0, S, S)
    ref = _reference((kind, dt, D, Hq, Hkv, S), do, q, k, v, scale, span_ref.global_mask(S, cu, pairs))
    out, lse, kinds = _fwd(q, k, v, scale, False, span=span)
    assert kinds and set(kinds) <= _WAVE_FWD, kinds
    grads, kinds = _bwd(do, q, k, v, ref, scale, False, span=span, dkdv_heads=dkdv_heads)
    assert {"dkdv_wave8", "dq_wave8"} <= set(kinds) <= _WAVE_BWD, kinds
    _check(out, lse, grads, ref, dt, Hq // Hkv, f"{dt} D{D} H{Hq}/{Hkv} heads/item {dkdv_heads} S{S} {kind}")


# ---- 2. ring blocks: below the diagonal (a left bound, every row_hi = Sk) and ABOVE it (a span across the shard boundary) ---------
def ring_block_case(where, dt, D):
    """256 rows against 512 keys, host side: (cu, spans, row0, key0, S_total, needle inputs).
    below: rows = global [512, 768), keys = [0, 512); documents end at 200, 449, 520: rows from 520 on see nothing.
    above: rows = global [0, 256), keys = [256, 768); the span [100, 300) crosses the boundary: rows 100 .. 255 see the keys
           256 .. 299 (local 0 .. 43), every other row sees nothing.  Needles on the last key inside and the first behind
           (local 43, 44) for the first rows of the span, and on local key 0 for row 99, the last row in front of it."""
    if where == "below":
        cu, spans, row0, key0 = [0, 200, 449, 520, 768], [(450, 460), (600, 768)], 512, 0
        edges = [(r, j) for r in (0, 1, 7) for j in (448, 449)] + [(8, 449)]
    else:
        cu, spans, row0, key0 = None, [(10, 20), (100, 300), (400, 500)], 0, 256
        edges = [(r, j) for r in (100, 101, 255) for j in (0, 43, 44)] + [(99, 0), (99, 43)]
    return cu, spans, row0, key0, 768, needle_inputs.make(256, 512, 4, 1, D, dt, C=8, seed=5 + D, edges=edges)


@pytest.mark.parametrize("dt,D", [("bfloat16", 128), ("float16", 64), ("bfloat16", 32)], ids=lambda v: str(v))
@pytest.mark.parametrize("mode", ["plain", "merge_in", "interleave"])
@pytest.mark.parametrize("where", ["below", "above"])
def test_ring_blocks(dev, dt, D, mode, where):
    from yunchang_amd import _C
    cu, spans, row0, key0, S_total, nd = ring_block_case(where, dt, D)
    q, k, v, do = [torch.from_numpy(x.astype(np.float32)).to(getattr(torch, dt)).to(dev) for x in (nd.q, nd.k, nd.v, nd.do)]
    Sq, Sk = q.shape[1], k.shape[1]
    span, host = _arrays(dev, cu, spans, row0, Sq, key0, Sk, S_total)
    empty_rows = host[0] >= host[1]
    assert empty_rows.any() and not empty_rows.all()              # rows that see nothing are in the launch
    full = span_ref.global_mask(S_total, cu, spans)[:, row0:row0 + Sq, key0:key0 + Sk]
    mask = span_ref.block_mask(host[0], host[1], Sq, Sk)
    assert torch.equal(mask, full) and torch.equal(span_ref.mask_of_keys(host[2], host[3], Sq, Sk), full)
    scale = D ** -0.5
    ref = span_ref.ref_bwd(do, q, k, v, scale, mask, out_dtype=q.dtype)
    what = f"{where} {dt} D{D} {mode}"
    if mode == "merge_in":
        g = torch.Generator().manual_seed(3)
        k0, v0 = (torch.randn(1, 128, 1, D, generator=g).to(q.dtype).to(dev) for _ in range(2))
        acc = torch.empty(q.shape, dtype=torch.float32, device=dev)
        lse = torch.empty((1, 4, Sq), dtype=torch.float32, device=dev)
        out = torch.full_like(q, float("nan"))
        _C.flash_fwd(q, k0, v0, scale, False, lse, out=out, acc=acc, final_begin=0, final_end=0, family="wave32")
        _C.flash_fwd(q, k, v, scale, False, lse, out=out, acc=acc, merge_in=True, final_begin=0, final_end=100, span=span)
        m2 = torch.cat([torch.ones(1, Sq, 128, dtype=torch.bool), mask], dim=2)
        want = span_ref.ref_fwd(q, torch.cat([k0, k], 1), torch.cat([v0, v], 1), scale, m2)
        assert_close(out[:, :100], want[0][:, :100], *TOL[dt]["out"], f"{what} out (final rows)")
        assert_close(acc[:, 100:], want[0][:, 100:], *TOL[dt]["out"], f"{what} acc (the other rows)")
        assert_close(lse, want[1], 2e-3, 1e-4, f"{what} lse")
        return
    kw = dict(interleave=True) if mode == "interleave" else {}
    out, lse, kinds = _fwd(q, k, v, scale, False, span=span, **kw)
    assert kinds and set(kinds) <= _WAVE_FWD, kinds
    empty = torch.from_numpy(empty_rows).to(dev)
    assert bool((out[0, empty] == 0).all()) and bool(torch.isneginf(lse[0, :, empty]).all()), "rows that see nothing: out = 0, lse = -inf"
    grads, kinds = _bwd(do, q, k, v, ref, scale, False, span=span, **kw)
    assert bool((grads[0][0, empty] == 0).all()), "rows that see nothing: dq = 0"
    _check(out, lse, grads, ref, dt, 4, what)


def test_a_launch_that_sees_nothing(dev):
    """Every row empty: out = 0, lse = -inf, zero gradients."""
    D, S = 64, 320
    q, k, v, do = _inputs(dev, S, 4, 1, D, "bfloat16", "alone")
    z = torch.zeros(S, dtype=torch.int32, device=dev)
    span = (z, z, torch.full((S,), S, dtype=torch.int32, device=dev), z)
    out, lse, _ = _fwd(q, k, v, D ** -0.5, False, span=span)
    assert bool((out == 0).all()) and bool(torch.isneginf(lse).all())
    ref = (torch.zeros_like(q, dtype=torch.float64), torch.full_like(lse, float("-inf"), dtype=torch.float64))
    grads, _ = _bwd(do, q, k, v, ref, D ** -0.5, False, span=span)
    assert all(bool((g == 0).all()) for g in grads)


# ---- 3. bit-identity ---------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("D,S", [(128, 1280), (64, 320)])
def test_null_row_hi_is_the_document_entry(dev, D, S):
    """row_hi == NULL (backward: and key_lo == NULL) is exactly usp_flash_fwd_doc / usp_flash_bwd_doc on the remaining arrays, and
    with everything NULL the plain launch: the same kernels, the same bits."""
    from yunchang_amd.ring import doc_blocks
    dt = "bfloat16"
    q, k, v, do = _inputs(dev, S, 4, 1, D, dt, "alone")
    scale = D ** -0.5
    rl, kh = (torch.from_numpy(a).to(dev) for a in doc_blocks.block_arrays(CU_DOCS[S], 0, S, 0, S))
    ref = _reference(("alone", dt, D, 4, 1, S), do, q, k, v, scale, span_ref.global_mask(S, None, SPANS[S]))
    for doc, span, what in (((rl, kh), (rl, None, None, kh), "NULL row_hi / key_lo"), (None, (None, None, None, None), "everything NULL")):
        f0 = _fwd(q, k, v, scale, True, doc=doc, family="wave32")
        b0 = _bwd(do, q, k, v, ref, scale, True, doc=doc, family="wave32", splits=(0, 0))
        if span[0] is None:
            from yunchang_amd import _C     # (span_value turns four Nones into "off": call the entry points themselves)
            f1, b1 = _raw_span_call(dev, q, k, v, do, ref, scale, True)
        else:
            f1 = _fwd(q, k, v, scale, True, span=span, family="wave32")
            b1 = _bwd(do, q, k, v, ref, scale, True, span=span, family="wave32", splits=(0, 0))
        assert f1[2] == f0[2] and b1[1] == b0[1], (what, f1[2], f0[2], b1[1], b0[1])
        for a, c, name in zip(f1[:2] + b1[0], f0[:2] + b0[0], ("out", "lse", "dq", "dk", "dv")):
            assert torch.equal(_bits(a), _bits(c)), f"{what}: {name} differs in bits"


def _raw_span_call(dev, q, k, v, do, ref, scale, causal):
    """usp_flash_fwd_span / usp_flash_bwd_span with every array NULL, on argument blocks filled as flash_fwd / flash_bwd fill them."""
    from yunchang_amd import _C
    out = torch.full_like(q, float("nan"))
    lse = torch.full((q.shape[0], q.shape[2], q.shape[1]), float("nan"), dtype=torch.float32, device=dev)
    a = _C._fwd_args(q, k, v, scale, causal, lse, out, None, False, 0, None, False, 0, None, _C.USP_FORCE_WAVE32, None, None)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(None)
    assert _C._span_entry("usp_flash_fwd_span")(ctypes.byref(a), null, 0, null, 0, stream) == 0
    fk = _C.last_launch_kinds()
    lse_in = ref[1].to(torch.float32)
    delta = torch.empty_like(lse_in)
    _C.bwd_delta(do, ref[0].to(q.dtype), delta)
    g = [torch.full(t.shape, float("nan"), dtype=torch.float32, device=dev) for t in (q, k, v)]
    b = _C.UspBwdArgs()
    b.dtype, b.B, b.Sq, b.Sk, b.Hq, b.Hkv, b.D = _C.dtype_code(q.dtype), q.shape[0], q.shape[1], k.shape[1], q.shape[2], k.shape[2], q.shape[3]
    b.causal, b.softmax_scale = int(causal), scale
    b.dout, b.q, b.k, b.v = _C._t4(do), _C._t4(q), _C._t4(k), _C._t4(v)
    b.lse, b.lse_stride_b, b.lse_stride_h = _C._lse3(lse_in)
    b.delta, b.delta_stride_b, b.delta_stride_h = _C._lse3(delta)
    b.dq, b.dk, b.dv = _C._t4(g[0]), _C._t4(g[1]), _C._t4(g[2])
    b.flags = _C.USP_FORCE_WAVE32
    need = _C.load().usp_flash_bwd_workspace_bytes(ctypes.byref(b))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    if need:
        b.workspace, b.workspace_bytes = ws.data_ptr(), need
    assert _C._span_entry("usp_flash_bwd_span")(ctypes.byref(b), null, 0, null, 0, null, 0, null, 0, stream) == 0
    return (out, lse, fk), (tuple(g), _C.last_launch_kinds())


@pytest.mark.parametrize("D,S", [(128, 1280), (64, 320)])
def test_arrays_of_plain_causal_against_the_wave32_family(dev, D, S):
    """row_lo = 0, row_hi = i + 1 (and the transpose) describe plain causal attention: the span kernels against the causal
    wave32 kernels.  Expected: agreement within the tolerances; whether the bits are the same is printed, not asserted (the span
    kernels reach the diagonal through the non-causal body: another instruction stream)."""
    dt = "bfloat16"
    q, k, v, do = _inputs(dev, S, 4, 1, D, dt, "alone")
    scale = D ** -0.5
    i = torch.arange(S, dtype=torch.int32, device=dev)
    span = (torch.zeros_like(i), i + 1, i.clone(), torch.full_like(i, S))
    causal_mask = torch.tril(torch.ones(S, S, dtype=torch.bool))[None]
    ref = _reference(("causal", dt, D, 4, 1, S), do, q, k, v, scale, causal_mask)
    f0 = _fwd(q, k, v, scale, True, family="wave32")
    b0 = _bwd(do, q, k, v, ref, scale, True, family="wave32", splits=(0, 0))
    f1 = _fwd(q, k, v, scale, False, span=span)
    b1 = _bwd(do, q, k, v, ref, scale, False, span=span)
    same = {name: bool(torch.equal(_bits(a), _bits(c)))
            for a, c, name in zip(f1[:2] + b1[0], f0[:2] + b0[0], ("out", "lse", "dq", "dk", "dv"))}
    print(f"[span-plain-causal-bits] D{D} S{S} same bits: {same}")
    _check(f1[0], f1[1], b1[0], ref, dt, 4, f"plain causal through the span kernels D{D} S{S}")
    _check(f0[0], f0[1], b0[0], ref, dt, 4, f"plain causal wave32 D{D} S{S}")


# ---- 4. refusals on the device: nothing launched, nothing written ------------------------------------------------------------------
def test_refusals_launch_nothing(dev):
    from yunchang_amd import _C
    D, S = 64, 320
    q, k, v, do = _inputs(dev, S, 4, 1, D, "bfloat16", "alone")
    span, _ = _arrays(dev, None, SPANS[S], 0, S, 0, S, S)
    for causal, kw in ((True, {}), (False, dict(window=(16, 0))), (False, dict(softcap=30.0)), (False, dict(shift=0)),
                       (False, dict(family="row64"))):
        out = torch.full_like(q, 7.0)
        lse = torch.full((1, 4, S), 7.0, dtype=torch.float32, device=dev)
        with pytest.raises(RuntimeError, match="not supported|unsupported"):
            _C.flash_fwd(q, k, v, D ** -0.5, causal, lse, out=out, span=span, **kw)
        torch.cuda.synchronize()
        assert _C.last_launch_kinds() == () and bool((out == 7.0).all()) and bool((lse == 7.0).all()), kw
        g = [torch.full(t.shape, 7.0, dtype=torch.float32, device=dev) for t in (q, k, v)]
        with pytest.raises(RuntimeError, match="not supported|unsupported"):
            _C.flash_bwd(do, q, k, v, lse, lse, *g, D ** -0.5, causal, span=span, **kw)
        torch.cuda.synchronize()
        assert _C.last_launch_kinds() == () and all(bool((t == 7.0).all()) for t in g), kw
    # a backward launch that is not skipped and lacks one of its two arrays: invalid argument; skipping that launch lifts it
    lse = torch.zeros((1, 4, S), dtype=torch.float32, device=dev)
    g = [torch.full(t.shape, 7.0, dtype=torch.float32, device=dev) for t in (q, k, v)]
    with pytest.raises(RuntimeError, match="invalid"):
        _C.flash_bwd(do, q, k, v, lse, lse, *g, D ** -0.5, False, span=(span[0], span[1], None, span[3]))
    assert _C.last_launch_kinds() == () and all(bool((t == 7.0).all()) for t in g)
    _C.flash_bwd(do, q, k, v, lse, lse, g[0], None, None, D ** -0.5, False, span=(span[0], span[1], None, None), only="dq")
    assert _C.last_launch_kinds() == ("dq_wave8",)


# ---- 5. every tensor in a strided layout of its own, the arrays as views into one poisoned buffer ----------------------------------
def test_independent_layouts(dev):
    from layout_util import Arena, blank, draw_layout, place
    from yunchang_amd import _C
    dt, D, S = "bfloat16", 64, 320
    q, k, v, do = _inputs(dev, S, 4, 1, D, dt, "in-docs")
    scale = D ** -0.5
    cu, bidir, pairs = _kind("in-docs", S)
    _, host = _arrays(dev, cu, bidir, 0, S, 0, S, S)
    poison = np.int32(0x40000000)
    gap = 37                                                       # odd offsets: the arrays are only 4-byte aligned
    buf = np.full(4 * (S + gap) + gap, poison, dtype=np.int32)
    for n, a in enumerate(host):
        buf[gap + n * (S + gap): gap + n * (S + gap) + S] = a
    dbuf = torch.from_numpy(buf).to(dev)
    span = tuple(dbuf[gap + n * (S + gap): gap + n * (S + gap) + S] for n in range(4))
    ref = _reference(("in-docs", dt, D, 4, 1, S), do, q, k, v, scale, span_ref.global_mask(S, cu, pairs))
    rs = np.random.RandomState(12)
    arena = Arena(dev)
    pq, pk, pv, pdo = (place(t, draw_layout(rs, "in16", 1), arena, n) for t, n in ((q, "q"), (k, "k"), (v, "v"), (do, "dout")))
    out = blank(q.shape, q.dtype, draw_layout(rs, "out16", 1), arena, "out")
    lse = blank((1, 4, S), torch.float32, draw_layout(rs, "lse", 1), arena, "lse")
    _C.flash_fwd(pq, pk, pv, scale, False, lse, out=out, span=span)
    delta = blank((1, 4, S), torch.float32, draw_layout(rs, "lse", 1), arena, "delta")
    plse = place(ref[1].to(torch.float32), draw_layout(rs, "lse", 1), arena, "lse_in")
    _C.bwd_delta(pdo, place(ref[0].to(q.dtype), draw_layout(rs, "in16", 1), arena, "o"), delta)
    dq, dk, dv = (blank(t.shape, torch.float32, draw_layout(rs, "f32", 1), arena, n) for t, n in ((q, "dq"), (k, "dk"), (v, "dv")))
    _C.flash_bwd(pdo, pq, pk, pv, plse, delta, dq, dk, dv, scale, False, span=span)
    torch.cuda.synchronize()
    assert arena.untouched(), arena.violations()
    assert arena.unchanged()
    assert torch.equal(dbuf.cpu(), torch.from_numpy(buf)), "the arrays' buffer was written"
    _check(out, lse, (dq, dk, dv), ref, dt, 4, "independent layouts")


# ---- 6. the public paths, at a padded head dim -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nccl_single():
    import os
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29741")
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
    cu = [CU_AROUND[S], [0, 1, 100, 319, 320]]                  # one list per batch entry
    spans = [SPANS[S], [(1, 60), (100, 102), (200, 319)]]
    ref = span_ref.ref_bwd(do, q, k, v, D ** -0.5, span_ref.global_mask(S, cu, spans, B), out_dtype=q.dtype)
    tq, tk, tv = (t.clone().requires_grad_(True) for t in (q, k, v))
    if path == "hip_attn_func":
        out = hip_attn_func(tq, tk, tv, causal=True, cu_doclens=cu, bidirectional=spans)
    else:
        Y.set_seq_parallel_pg(1, 1, 0, 1)
        out = Y.LongContextAttention(ring_impl_type="basic", attn_type=Y.AttnType.HIP)(tq, tk, tv, causal=True, cu_doclens=cu,
                                                                                      bidirectional=spans)
    out.backward(do)
    _check(out, ref[1].float(), (tq.grad, tk.grad, tv.grad), ref, dt, Hq // Hkv, path)


# ---- 7. the basic ring on virtual ranks, a span across a shard boundary and one longer than a shard ---------------------------------
@pytest.mark.timeout(600)
def test_basic_ring_on_virtual_ranks(dev, nccl_single, monkeypatch):
    """S_total = 1024 on P = 4 (shards of 256): the span [200, 300) straddles the first boundary (block (rank 0, keys of rank 1)
    above the diagonal is live), [500, 1000) is longer than a shard (rank 1 sees the keys of ranks 2 and 3, rank 2 those of
    rank 3): the planned direct transport, forward and backward."""
    import yunchang_amd.ring.ring_flash_attn as R
    from yunchang_amd.ring import doc_blocks
    from virtual_grid import VirtualGridPairwise, patch_dist, run_grid
    P, S, Hq, Hkv, D = 4, 1024, 4, 2, 64
    cu, spans = [0, 100, 1024], [(10, 50), (200, 300), (500, 1000)]
    plan = doc_blocks.parse_plan(cu, spans, 1, S)
    rows, scale = S // P, D ** -0.5
    assert doc_blocks.spans_cross_shards(plan, rows, P)
    assert doc_blocks.SpanRingPlan(plan, rows, P, 0).steps == [0, 3] and doc_blocks.SpanRingPlan(plan, rows, P, 1).steps == [0, 1, 2, 3]
    grid = VirtualGridPairwise(1, P, nccl_single)
    patch_dist(monkeypatch, grid)
    g = torch.Generator().manual_seed(41)
    q, k, v, do = (torch.randn(1, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv, Hq))
    loc = [[t[:, r * rows:(r + 1) * rows].contiguous() for t in (q, k, v, do)] for r in range(P)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(P)]
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        _, rpg = grid.groups_of(r)
        lq, lk, lv, ldo = loc[r]
        with torch.cuda.stream(streams[r]):
            out, lse = R.ring_flash_attn_forward(rpg, lq, lk, lv, scale, causal=True, cu_doclens=plan)
            return [out] + list(R.ring_flash_attn_backward(rpg, ldo, lq, lk, lv, out, lse, scale, causal=True, cu_doclens=plan))
    res = run_grid(grid, P, rank_fn)
    torch.cuda.synchronize()
    ref = span_ref.ref_bwd(do, q, k, v, scale, span_ref.global_mask(S, cu, spans), out_dtype=q.dtype)
    for r in range(P):
        sl = slice(r * rows, (r + 1) * rows)
        for got, want, tol, name in ((res[r][0], ref[0], TOL["bfloat16"]["out"], "out"), (res[r][1], ref[2], grad_tol("bfloat16", 2), "dq"),
                                     (res[r][2], ref[3], grad_tol("bfloat16", 2), "dk"), (res[r][3], ref[4], grad_tol("bfloat16", 2), "dv")):
            assert_close(got, want[:, sl], *tol, f"ring {P} rank {r} {name}")


# ---- 8. a small seeded fuzz: random documents and spans on ragged shapes -----------------------------------------------------------
def fuzz_case(seed):
    """(S, Hq, Hkv, D, dt, cu | None, spans): S in [2, 700), at least one span of length >= 2, spans inside documents."""
    rs = np.random.RandomState(7100 + seed)
    S = int(rs.randint(2, 700))
    D = (32, 64, 128)[seed % 3]
    dt = ("bfloat16", "float16")[(seed // 3) % 2]
    Hkv = int(rs.randint(1, 3))
    Hq = Hkv * (1, 2, 4)[int(rs.randint(3))]
    cu = None
    if seed % 2:
        inner = sorted(set(int(x) for x in rs.randint(1, S, size=int(rs.randint(1, 6))))) if S > 2 else []
        cu = [0] + [x for x in inner if 0 < x < S] + [S]
    bounds = cu or [0, S]
    spans = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        pos = a
        while pos < b - 1 and rs.rand() < 0.8:
            s = int(rs.randint(pos, b - 1))
            e = int(rs.randint(s + 1, b + 1))
            spans.append((s, e))
            pos = e
    if not any(e - s >= 2 for s, e in spans):                      # every case has a real span: the longest document, whole
        a, b = max(zip(bounds[:-1], bounds[1:]), key=lambda d: d[1] - d[0])
        spans = sorted([sp for sp in spans if sp[1] <= a or sp[0] >= b] + [(a, b)])
    return S, Hq, Hkv, D, dt, cu, spans


@pytest.mark.parametrize("seed", range(12))
def test_fuzz(dev, seed):
    S, Hq, Hkv, D, dt, cu, spans = fuzz_case(seed)
    assert any(e - s >= 2 for s, e in spans)
    nd = needle_inputs.make(S, S, Hq, Hkv, D, dt, C=8, seed=seed, edges=[(r, j) for r, j in span_ref.needle_edges(spans, S, cu)])
    q, k, v, do = [torch.from_numpy(x.astype(np.float32)).to(getattr(torch, dt)).to(dev) for x in (nd.q, nd.k, nd.v, nd.do)]
    scale = D ** -0.5
    span, host = _arrays(dev, cu, spans, 0, S, 0, S, S)
    mask = span_ref.global_mask(S, cu, spans)
    assert torch.equal(span_ref.block_mask(host[0], host[1], S, S), mask)
    ref = span_ref.ref_bwd(do, q, k, v, scale, mask, out_dtype=q.dtype)
    out, lse, _ = _fwd(q, k, v, scale, False, span=span)
    grads, _ = _bwd(do, q, k, v, ref, scale, False, span=span)
    _check(out, lse, grads, ref, dt, Hq // Hkv, f"fuzz {seed}: S{S} H{Hq}/{Hkv} D{D} {dt} cu {cu} spans {spans}")
