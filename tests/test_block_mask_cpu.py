"""Block-sparse attention (block_mask=) without a GPU: the fp64 reference of the GPU tests pinned three ways, mutants of it that
must fail at the GPU tests' tolerances, the argument logic of the Python layers on a recording backend, and gloo grids (basic
ring 2 and 4, hybrid 2 x 2) on a block backend that applies each launch's sub-mask through tests/block_mask_ref.py."""
import numpy as np
import pytest
import torch

import attn_ref_torch as A
import block_mask_ref as R
import interval_ref as I
from golden_util import TOL, close_mask, grad_tol, make_inputs

B, S, HQ, HKV, D = 2, 640, 4, 2, 32
SCALE = D ** -0.5


@pytest.fixture(scope="module")
def data():
    return [torch.from_numpy(x).double() for x in make_inputs(B, S, HQ, HKV, D, seed=3)]      # q, k, v, dout


# ---- 1. the reference, pinned ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
def test_all_true_mask_is_dense_attention(data, causal):
    q, k, v, do = data
    m = torch.ones(5, 5, dtype=torch.bool)
    out, lse = R.ref_fwd(q, k, v, SCALE, m, causal)
    o2, l2 = A.ref_fwd(q, k, v, SCALE, causal)
    assert (out - o2).abs().max() < 1e-12 and (lse - l2).abs().max() < 1e-12
    for a, b in zip(R.ref_bwd(do, q, k, v, out, lse, SCALE, m, causal), A.ref_bwd(do, q, k, v, o2, l2, SCALE, causal)):
        assert (a - b).abs().max() < 1e-10


@pytest.mark.parametrize("kind", ["documents", "band"])
def test_interval_masks_match_interval_ref(data, kind):
    """Documents whose lengths are multiples of 128 (a block-diagonal mask, causal) and a band of two blocks (causal) are
    interval masks: the same numbers as tests/interval_ref.py with the equivalent row_lo / row_hi."""
    q, k, v, do = data
    rows = np.arange(S)
    if kind == "documents":
        cu = [0, 256, 384, 640]
        m = torch.zeros(5, 5, dtype=torch.bool)
        for s, e in zip(cu[:-1], cu[1:]):
            m[s // 128:e // 128, s // 128:e // 128] = True
        lo, hi = I.bounds(S, cu)
    else:
        blk = torch.arange(5)
        m = (blk[:, None] - blk[None, :]).abs() <= 1
        lo, hi = np.clip((rows // 128 - 1) * 128, 0, S), rows + 1
    out, lse = R.ref_fwd(q, k, v, SCALE, m, True)
    o2, l2 = I.ref_fwd(q, k, v, SCALE, lo, hi)
    assert (out - o2).abs().max() < 1e-12 and (lse - l2).abs().max() < 1e-12
    for a, b in zip(R.ref_bwd(do, q, k, v, out, lse, SCALE, m, True), I.ref_bwd(do, q, k, v, o2, l2, SCALE, lo, hi)):
        assert (a - b).abs().max() < 1e-10


def test_rows_that_see_nothing(data):
    q, k, v, do = data
    m = torch.ones(5, 5, dtype=torch.bool)
    m[2, :] = False
    out, lse = R.ref_fwd(q, k, v, SCALE, m, False)
    assert bool((out[:, 256:384] == 0).all()) and bool((lse[:, :, 256:384] == float("-inf")).all())
    assert bool(torch.isfinite(lse[:, :, :256]).all())
    dq = R.ref_bwd(do, q, k, v, out, lse, SCALE, m, False)[0]
    assert bool((dq[:, 256:384] == 0).all())


# ---- 2. mutants: each must fail the comparison the GPU tests make, the unmutated reference passes with every case counted ----------
def _passes(got, want, dt="bfloat16"):
    """The GPU tests' verdict (tests/test_gpu_block_mask.py: check) on (out, lse, dq, dk, dv)."""
    tols = [TOL[dt]["out"], (2e-3, 1e-4)] + [grad_tol(dt, 2)] * 3
    return all(bool(close_mask(g, w, *t)[0].all()) for g, w, t in zip(got, want, tols))


def test_mutants_fail(data):
    q, k, v, do = data
    g = torch.Generator().manual_seed(5)
    mask = torch.rand(B, HQ, 5, 5, generator=g) < 0.5
    mask |= torch.eye(5, dtype=torch.bool)
    mask[:, 1] = ~mask[:, 0]                       # the heads differ everywhere but ...
    mask[:, 1] |= torch.eye(5, dtype=torch.bool)   # ... on the diagonal
    want = R.ref_all(do, q, k, v, SCALE, mask, True)
    counted = 0
    assert _passes(R.ref_all(do, q, k, v, SCALE, mask.clone(), True), want)
    flipped = mask.clone()
    flipped[1, 2, 3, 1] = ~flipped[1, 2, 3, 1]                                   # one bit below the diagonal
    mutants = {"one bit flipped": dict(mask=flipped),
               "head h read for head h + 1": dict(mask=torch.roll(mask, 1, dims=1)),
               "transposed lists from the untransposed mask": dict(mask=mask, kv_mask=mask.transpose(-1, -2)),
               "diagonal block full": dict(mask=mask, diag_full=True)}
    for name, kw in mutants.items():
        m = kw.pop("mask")
        causal = True
        if name.startswith("transposed"):          # (a causal transpose would be cut by the diagonal: the full mask shows it)
            causal = False
            base = R.ref_all(do, q, k, v, SCALE, mask, False)
            assert _passes(R.ref_all(do, q, k, v, SCALE, mask, False), base)
            assert not _passes(R.ref_all(do, q, k, v, SCALE, m, causal, **kw), base), name
        else:
            assert not _passes(R.ref_all(do, q, k, v, SCALE, m, causal, **kw), want), name
        counted += 1
    assert counted == 4


# ---- 3. argument logic --------------------------------------------------------------------------------------------------------------
class Recorder:
    """A block backend that records its flash calls and computes nothing."""
    name = "recorder"

    def __init__(self):
        self.calls = []

    def fwd(self, q, k, v, scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None, **kw):
        self.calls.append(("fwd", causal, merge_in, kw))
        lse.zero_()
        if out is not None:
            out.zero_()

    def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, scale, causal, **kw):
        self.calls.append(("bwd", causal, kw))

    def delta(self, dout, out, delta):
        delta.zero_()


@pytest.fixture
def recorder():
    from yunchang_amd.kernels import attention as K
    rec = Recorder()
    prev = K.set_block_backend(rec)
    yield rec
    K.set_block_backend(prev)


def _small():
    q = torch.zeros(1, 256, 4, 32, dtype=torch.bfloat16)
    k = torch.zeros(1, 256, 2, 32, dtype=torch.bfloat16)
    return q, k, k.clone(), torch.ones(2, 2, dtype=torch.bool)


@pytest.mark.parametrize("name,kw", [("window_size", dict(window_size=(64, 0))), ("softcap", dict(softcap=30.0)),
                                     ("alibi_slopes", dict(alibi_slopes=torch.ones(4))), ("dropout_p", dict(dropout_p=0.1)),
                                     ("sinks", dict(sinks=torch.zeros(4))), ("cu_doclens", dict(cu_doclens=[0, 128, 256])),
                                     ("bidirectional", dict(bidirectional=[(0, 8)]))])
def test_refused_beside_every_other_option(recorder, name, kw):
    """Judged in one place (kernels/features.py: block_mask_alone), before any tensor is read: the entry points and the layers."""
    from yunchang_amd.kernels.attention import hip_attn_forward, hip_attn_func
    from yunchang_amd.ring.ring_flash_attn import ring_flash_attn_func
    from yunchang_amd.ring.zigzag_ring_flash_attn import zigzag_ring_flash_attn_func
    q, k, v, m = _small()
    msg = f"block_mask together with {name} is not supported by the HIP attention kernels"
    for fn in (hip_attn_forward, hip_attn_func, ring_flash_attn_func, zigzag_ring_flash_attn_func):
        with pytest.raises(NotImplementedError) as e:
            fn(q, k, v, causal=True, block_mask=m, **kw)
        assert str(e.value) == msg
    assert recorder.calls == []


def test_other_refusals(recorder):
    from yunchang_amd.hybrid.async_attn_layer import AsyncLongContextAttention
    from yunchang_amd.kernels.attention import hip_attn_forward
    from yunchang_amd.ring import front_end as F
    from yunchang_amd.ring.ring_flash_attn_varlen import ring_flash_attn_varlen_func
    q, k, v, m = _small()
    with pytest.raises(NotImplementedError, match="same length"):
        hip_attn_forward(q, k[:, :128], v[:, :128], block_mask=m)
    for bad, exc in ((m.float(), ValueError), (torch.ones(3, 3, dtype=torch.bool), ValueError),
                     (torch.ones(3, 2, 2, dtype=torch.bool), ValueError)):
        with pytest.raises(exc):
            hip_attn_forward(q, k, v, block_mask=bad)
    with pytest.raises(NotImplementedError, match="variable-length.*ring_flash_attn_func"):
        ring_flash_attn_varlen_func(q[0], k[0], v[0], torch.tensor([0, 256], dtype=torch.int32), 256, block_mask=m)
    with pytest.raises(NotImplementedError, match="AsyncLongContextAttention.*LongContextAttention"):
        AsyncLongContextAttention.forward(None, q, k, v, block_mask=m)

    class G4:                                   # a ring group of degree 4, as group_info reads it
        pass
    import yunchang_amd.ring.front_end as FE
    orig = FE.group_info
    FE.group_info = lambda dist, group: (4, 1)
    try:
        with pytest.raises(NotImplementedError, match="zigzag and stripe rings.*basic ring"):
            F._place_block_mask(F.DENSE_RING, q, k, F.BlockMask(torch.ones(8, 8, dtype=torch.bool)), G4())
        with pytest.raises(NotImplementedError, match="multiple of 128"):
            F._place_block_mask(F.BASIC_RING, q[:, :200], k[:, :200], F.BlockMask(torch.ones(7, 7, dtype=torch.bool)), G4())
        F._place_block_mask(F.BASIC_RING, q, k, F.BlockMask(torch.ones(8, 8, dtype=torch.bool)), G4())
        with pytest.raises(ValueError):
            F._place_block_mask(F.BASIC_RING, q, k, F.BlockMask(torch.ones(2, 2, dtype=torch.bool)), G4())
    finally:
        FE.group_info = orig
    assert recorder.calls == []


def test_none_is_the_call_without_the_keyword(recorder):
    from yunchang_amd.kernels.attention import hip_attn_backward, hip_attn_forward
    q, k, v, m = _small()
    hip_attn_forward(q, k, v, causal=True)
    hip_attn_forward(q, k, v, causal=True, block_mask=None)
    out, lse = hip_attn_forward(q, k, v, causal=True, block_mask=m)
    assert recorder.calls[0] == recorder.calls[1] and "bsp" not in recorder.calls[0][3]
    assert recorder.calls[2][3]["bsp"] is m
    g = [torch.empty_like(t) for t in (q, k, v)]
    del recorder.calls[:]
    hip_attn_backward(q, q, k, v, out, lse, *g, bwd_causal=True)
    hip_attn_backward(q, q, k, v, out, lse, *g, bwd_causal=True, block_mask=None)
    hip_attn_backward(q, q, k, v, out, lse, *g, bwd_causal=True, block_mask=m)
    a, b, c = recorder.calls
    assert a[1:2] == b[1:2] and set(a[2]) == set(b[2]) and "bsp" not in a[2] and c[2]["bsp"] is m


@pytest.mark.parametrize("P", [2, 4])
def test_ring_views_follow_the_slice_formula(P):
    """What the basic ring hands the launch of (rank r, step s): mask[..., r n:(r + 1) n, kr n:(kr + 1) n], kr = r - s mod P,
    n = S / 128 -- by data_ptr, shape and strides: a view, no copy."""
    from yunchang_amd.ring.front_end import BlockMask
    from yunchang_amd.ring.ring_flash_attn import _bsp_kw
    S_loc = 256
    n, nb = S_loc // 128, P * S_loc // 128
    mask = torch.rand(2, 4, nb, nb) < 0.5
    assert _bsp_kw(None, 0, P, 0, S_loc) == {}
    for r in range(P):
        for step in range(P):
            kr = (r - step) % P
            view = _bsp_kw(BlockMask(mask), r, P, step, S_loc)["bsp"]
            assert tuple(view.shape) == (2, 4, n, n) and view.stride() == mask.stride()
            assert view.data_ptr() == mask.data_ptr() + (r * n * nb + kr * n) * mask.element_size()
            assert torch.equal(view, mask[:, :, r * n:(r + 1) * n, kr * n:(kr + 1) * n])
    assert _bsp_kw(BlockMask(mask), 0, 1, 0, P * S_loc)["bsp"] is mask


def test_ulysses_cuts_the_heads():
    from yunchang_amd.comm.all_to_all import local_block_mask, local_heads
    H, P = 8, 4
    m4 = torch.rand(2, H, 3, 3) < 0.5
    for rank in range(P):
        hs = local_heads(H, P, rank)
        cut = local_block_mask(m4, H, P, rank)
        assert torch.equal(cut, m4[:, hs]) and cut.data_ptr() == m4[:, hs].data_ptr()
        assert torch.equal(local_block_mask(m4[0], H, P, rank), m4[0, hs])
        assert local_block_mask(m4[:, :2], H, P, rank).shape[1] == 2            # over the local heads: as it is
        assert local_block_mask(m4[0, 0], H, P, rank) is not None and local_block_mask(m4[0, 0], H, P, rank).dim() == 2
    with pytest.raises(ValueError):
        local_block_mask(m4[:, :3], H, P, 0)
    assert local_block_mask(None, H, P, 0) is None


def test_helpers():
    from yunchang_amd import _C
    from yunchang_amd.kernels.attention import BLOCK_MASK_SIZE, expand_block_mask
    assert BLOCK_MASK_SIZE == _C.BLOCK_MASK_SIZE == 128
    m = torch.tensor([[True, False], [True, True]])
    assert expand_block_mask(m, 128) is m
    assert torch.equal(expand_block_mask(m, 256), torch.tensor([[1, 1, 0, 0], [1, 1, 0, 0], [1, 1, 1, 1], [1, 1, 1, 1]]).bool())
    with pytest.raises(ValueError):
        expand_block_mask(m, 192)
    u8, sb, sh, sr = _C.block_mask_value(torch.ones(2, 4, 6, 3, dtype=torch.bool)[:, :, ::2], 2, 4, 384, "cpu")
    assert u8.dtype == torch.uint8 and (sb, sh, sr) == (72, 18, 6)                # strides as they are: no copy
    assert _C.block_mask_value(torch.ones(3, 3, dtype=torch.bool), 2, 4, 384, "cpu")[1:] == (0, 0, 3)
    assert _C.block_mask_value(torch.ones(3, 6, dtype=torch.bool)[:, ::2], 2, 4, 384, "cpu")[3] == 3   # made contiguous once


# ---- 4. gloo grids in fp64: a block backend that applies the mask through block_mask_ref ------------------------------------------
from dist_util import run_distributed        # noqa: E402
from doc_ref import DocOracleBackend         # noqa: E402
from golden_util import assert_close         # noqa: E402

GB, GS, GHQ, GHKV, GD = 1, 512, 4, 2, 16
GSCALE = GD ** -0.5


def _grid_inputs():
    g = torch.Generator().manual_seed(29)
    q, k, v, do = (torch.randn(GB, GS, h, GD, generator=g).to(torch.bfloat16) for h in (GHQ, GHKV, GHKV, GHQ))
    mask = torch.rand(GB, GHQ, 4, 4, generator=g) < 0.5
    mask[:, :, 2, 1:] = False                     # row block 2 sees key block 0 only: empty in every other ring block
    mask |= torch.eye(4, dtype=torch.bool)
    mask[:, 1, 3, :] = False                      # head 1, row block 3: sees nothing at all
    return q, k, v, do, mask


class BlockOracleBackend(DocOracleBackend):
    """The oracle block backend with `bsp=` on fwd and bwd: the launch is computed in fp64 under tests/block_mask_ref.py's
    visibility of the sub-mask it was handed -- in the launch's own coordinates, with the launch's own `causal` -- and merged /
    accumulated the way the kernels' epilogues do.  A launch without the keyword is the wrapped oracle's.  Logs every such
    launch in `bsp_log`: (kind, causal, merge_in / accum_dq, data_ptr, shape, strides)."""

    def __init__(self):
        super().__init__()
        self.bsp_log = []

    def fwd(self, q, k, v, softmax_scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None,
            bsp=None, **kw):
        if bsp is None:
            return super().fwd(q, k, v, softmax_scale, causal, lse, out, acc, merge_in, final_begin, final_end, **kw)
        assert all(x is None for x in kw.values()), "a block-sparse launch carries no other option"
        self.bsp_log.append(("fwd", bool(causal), bool(merge_in), bsp.data_ptr(), tuple(bsp.shape), bsp.stride()))
        Sq = q.shape[1]
        o, l = R.ref_fwd(q, k, v, softmax_scale, bsp, bool(causal))
        if merge_in:
            old = lse.to(torch.float64)
            new = torch.logaddexp(old, l)
            fin = torch.isfinite(new)
            safe = torch.where(fin, new, torch.zeros_like(new))
            w_old = torch.where(fin, torch.exp(old - safe), torch.zeros_like(new))
            w_blk = torch.where(fin, torch.exp(l - safe), torch.zeros_like(new))
            o = acc.to(torch.float64) * w_old.transpose(1, 2)[..., None] + o * w_blk.transpose(1, 2)[..., None]
            l = new
        lse.copy_(l)
        fe = Sq if final_end is None else final_end
        for dst, rows in ((out, slice(final_begin, fe)), (acc, slice(0, final_begin)), (acc, slice(fe, Sq))):
            if dst is not None and rows.stop > rows.start:
                dst[:, rows].copy_(o[:, rows])

    def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale, causal, accum_dq=False, accum_dk=False, accum_dv=False,
            dq16=None, dk16=None, dv16=None, bsp=None, **kw):
        if bsp is None:
            return super().bwd(dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale, causal, accum_dq, accum_dk, accum_dv,
                               dq16, dk16, dv16, **kw)
        assert all(x is None for x in kw.values()), "a block-sparse launch carries no other option"
        self.bsp_log.append(("bwd", bool(causal), bool(accum_dq), bsp.data_ptr(), tuple(bsp.shape), bsp.stride()))
        B, Sq, Hq, D = q.shape
        Sk, Hkv = k.shape[1], k.shape[2]
        G = Hq // Hkv
        m4 = R.mask4(bsp, B, Hq, Sq)
        vis = torch.stack([R.visible(m4, b, 0, Sq, Sk, bool(causal)) for b in range(B)])            # (B, Hq, Sq, Sk)
        q64, do64 = q.to(torch.float64), dout.to(torch.float64)
        k64, v64 = (t.to(torch.float64).repeat_interleave(G, dim=2) for t in (k, v))
        s = torch.einsum("bihd,bjhd->bhij", q64, k64) * softmax_scale
        l = lse.to(torch.float64)[..., None]
        fin = torch.isfinite(l)
        p = torch.where(vis & fin, torch.exp(s - torch.where(fin, l, torch.zeros_like(l))), torch.zeros_like(s))
        ds = p * (torch.einsum("bihd,bjhd->bhij", do64, v64) - delta.to(torch.float64)[..., None]) * softmax_scale
        g = (torch.einsum("bhij,bjhd->bihd", ds, k64),
             torch.einsum("bhij,bihd->bjhd", ds, q64).reshape(B, Sk, Hkv, G, D).sum(3),
             torch.einsum("bhij,bihd->bjhd", p, do64).reshape(B, Sk, Hkv, G, D).sum(3))
        for val, d32, d16, accum in zip(g, (dq, dk, dv), (dq16, dk16, dv16), (accum_dq, accum_dk, accum_dv)):
            if accum:
                val = val + d32.to(torch.float64)
            if d16 is not None:
                d16.copy_(val)
            elif d32 is not None:
                d32.copy_(val)


def _grid_worker(rank, ws, ud, rd, causal):
    import yunchang_amd as Y
    from yunchang_amd.comm.all_to_all import local_block_mask
    from yunchang_amd.kernels import set_block_backend
    from yunchang_amd.ring import ring_flash_attn_func
    be = BlockOracleBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    q, k, v, do, mask = _grid_inputs()
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    loc = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in (q, k, v, do)]
    res = {"cases": {}}

    def run(fn, name):
        lv = [t.detach().clone().requires_grad_(True) for t in loc[:3]]
        out = fn(*lv)
        out.backward(loc[3])
        res["cases"][name] = [t.detach().float().numpy() for t in (out,) + tuple(x.grad for x in lv)]
    layer = Y.LongContextAttention(ring_impl_type="basic")
    del be.bsp_log[:]
    run(lambda a, b, c: layer(a, b, c, causal=causal, block_mask=mask), "layer")
    # the views the ring's forward and backward handed their launches, against the slice formula on the rank's head cut
    u, r = rank % ud, rank // ud
    base = local_block_mask(mask, GHQ, ud, u)
    n = (GS // rd) // 128
    steps = [s for s in range(rd) if not (causal and s > r)]
    want = {}
    for s in steps:
        kr = (r - s) % rd
        view = base[..., r * n:(r + 1) * n, kr * n:(kr + 1) * n] if rd > 1 else base
        want[s] = (bool(causal and s == 0), view.data_ptr(), tuple(view.shape), view.stride())
    fwd = [x for x in be.bsp_log if x[0] == "fwd"]
    bwd = [x for x in be.bsp_log if x[0] == "bwd"]
    res["fwd_views"] = [(x[1], x[3], x[4], x[5]) for x in fwd] == [want[s] for s in steps]
    res["fwd_merge"] = [x[2] for x in fwd] == [s > 0 for s in steps]
    res["bwd_views"] = sorted((x[1], x[3], x[4], x[5]) for x in bwd) == sorted(want.values())
    res["bwd_first_opens_dq"] = rd == 1 or ([x[2] for x in bwd].count(False) == 1)
    if ud == 1:
        run(lambda a, b, c: ring_flash_attn_func(a, b, c, causal=causal, block_mask=mask, group=Y.PROCESS_GROUP.RING_PG), "ring_func")
    if rd > 1:
        refused = []
        for impl in ("zigzag", "strip"):
            try:
                Y.LongContextAttention(ring_impl_type=impl)(*loc[:3], causal=causal, block_mask=mask)
                refused.append(False)
            except NotImplementedError as e:
                refused.append("basic ring" in str(e) and "block_mask" in str(e))
        res["refused"] = all(refused)
    return res


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("ud,rd", [(1, 2), (1, 4), (2, 2)], ids=lambda v: str(v))
def test_gloo_grids_against_the_unsharded_reference(ud, rd, causal):
    """Basic ring of degree 2 and 4 and a 2 x 2 hybrid on gloo, the real layer and ring code with autograd, every launch computed
    in fp64 by BlockOracleBackend from the view it was handed: equal to the single-process reference for the same global mask;
    and every (rank, step) launch of the real ring forward / backward got the view the slice formula names (data_ptr, shape,
    strides), the diagonal step causal, the others full, merge_in from the second step on."""
    import yunchang_amd as Y
    ws = ud * rd
    res = run_distributed(_grid_worker, ws, ud, rd, causal)
    q, k, v, do, mask = _grid_inputs()
    truth = R.ref_all(do, q, k, v, GSCALE, mask, causal)
    truth = (truth[0],) + tuple(truth[2:])
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    for rank in range(ws):
        want = [ext(t, rank, world_size=ws, rd=rd, ud=ud) for t in truth]
        for name, got in res[rank]["cases"].items():
            for g, w, what in zip(got, want, ("out", "dq", "dk", "dv")):
                tol = TOL["bfloat16"]["out"] if what == "out" else grad_tol("bfloat16", GHQ // GHKV)
                assert_close(g, w, *tol, f"grid {ud}x{rd} rank {rank} {name} {what}")
        for key in ("fwd_views", "fwd_merge", "bwd_views", "bwd_first_opens_dq"):
            assert res[rank][key], (rank, key)
        assert res[rank].get("refused", True)
