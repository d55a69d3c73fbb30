"""The gathered-key backward (csrc/usp_flash_bwd_gather.hip; include/usp_hip.h: USP_ATTN_KEY_INDEX_BWD) on the GPU: every element of dq,
dk and dv against fp64 autograd through tests/key_index_ref.py.  A dQ item is 128 rows, a list tile 64 entries, a streamed tile 64 rows."""
import pytest
import torch

import key_index_ref as R
from golden_util import TOL, assert_close
from test_gpu_key_index import _inputs, _lists, _strided

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
SHAPES = [(1, 320, 320, 4, 1, 128), (2, 192, 192, 2, 2, 64), (1, 77, 333, 3, 1, 128)]
_DOUT = {}


def _dout(q):
    if q.shape not in _DOUT:
        _DOUT[q.shape] = torch.randn(q.shape, generator=torch.Generator().manual_seed(7)).to(q.dtype).to(dev)
    return _DOUT[q.shape].to(q.dtype)


def _reference(q, k, v, dout, idx, left, scale=None):
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    out, _ = R.attention(qd, kd, vd, scale or q.shape[-1] ** -0.5, R.mask(q.shape[1], k.shape[1], idx, left))
    out.backward(dout.double())
    return qd.grad, kd.grad, vd.grad


def _window(left):
    return (-1, -1) if left is None else (left, 0)


def _backward(q, k, v, dout, idx, left):
    from yunchang_amd.kernels import hip_attn_backward, hip_attn_forward
    out, lse = hip_attn_forward(q, k, v, causal=True, window_size=_window(left), key_index=idx)
    g = [torch.empty_like(t) for t in (q, k, v)]
    hip_attn_backward(dout, q, k, v, out, lse, *g, 0.0, None, True, _window(left), key_index=idx)
    return g


def _compare(got, want, dt, what):
    for name, g, w in zip(("dq", "dk", "dv"), got, want):
        assert_close(g, w, *TOL[dt]["grad"], f"{what} {name}")


@pytest.mark.parametrize("left", [None, 0, 31])
@pytest.mark.parametrize("n", [1, 64, 65, 130])
@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gradients_against_fp64(shape, dt, n, left):
    """The first shape has four query heads with different lists on one KV head (the scatter's sum); flat head 1 is half absent, flat
    head 2 all absent: without a window its rows saw nothing and their dq is exactly 0."""
    from yunchang_amd import _C
    B, Sq, Sk, Hq, Hkv, D = shape
    q, k, v = _inputs(*shape, dt)
    idx, dout = _lists(B, Hq, n, Sk, 100 + n), _dout(q)
    got = _backward(q, k, v, dout, idx, left)
    kinds = _C.last_launch_kinds()
    assert "dq_gather" in kinds and "dkdv_gather" in kinds, kinds
    _compare(got, _reference(q, k, v, dout, idx, left), dt, f"{shape} {dt} n={n} left={left}")
    if left is None:
        b, h = divmod(2, Hq)
        assert (got[0][b, :, h] == 0).all(), "the all-absent head got a dq"


def test_needle_dv_is_exact_for_every_key_of_two_tiles_plus_one():
    """One listed key per head, dout in {-1, 0, 1}: p = 1 on the rows at or past the key, so dv[key] is the integer sum of their dout
    rows over the heads that list it (|.| <= 160: exact in fp32 and bf16); every other dv row and every unlisted dk row is exactly 0."""
    B, S, Hq, G, D = 1, 160, 2, 2, 64
    q, k, v = _inputs(B, S, S, Hq, Hq // G, D, "bfloat16")
    dout = torch.randint(-1, 2, q.shape, generator=torch.Generator().manual_seed(3)).to(q.dtype).to(dev)
    tol = TOL["bfloat16"]["grad"]
    for key in range(129):
        keys = [key, (key + 64) % 129]
        dq, dk, dv = _backward(q, k, v, dout, torch.tensor(keys, dtype=torch.int32, device=dev)[:, None], None)
        want = torch.zeros(S, D, device=dev)
        for h, kk in enumerate(keys):
            want[kk] += dout[0, kk:, h].float().sum(0)
        assert torch.equal(dv[0, :, 0].float(), want), f"key {key}: dv"
        unlisted = torch.ones(S, dtype=torch.bool, device=dev)
        unlisted[keys] = False
        assert (dk[0, unlisted] == 0).all(), f"key {key}: dk of an unlisted key"
        assert_close(dq, torch.zeros_like(dq), *tol, f"key {key} dq")
        assert_close(dk, torch.zeros_like(dk), *tol, f"key {key} dk")


@pytest.mark.parametrize("left", [None, 31])
def test_strided_views_in_poisoned_storage_and_a_guarded_workspace(left):
    from yunchang_amd import _C
    shape, dt, n = SHAPES[1], "bfloat16", 65
    B, Sq, Sk, Hq, Hkv, D = shape
    q, k, v = _inputs(*shape, dt)
    idx, dout = _lists(B, Hq, n, Sk, 5), _dout(q)
    from yunchang_amd.kernels import hip_attn_forward
    out, lse = hip_attn_forward(q, k, v, causal=True, window_size=_window(left), key_index=idx)
    delta = (dout.float() * out.float()).sum(-1).permute(0, 2, 1).contiguous()
    tdo, tq, tk, tv = (_strided(t, 8, float("nan")) for t in (dout, q, k, v))
    store = torch.full((B, Hq + 1, n + 9), 0x40000000, dtype=torch.int32, device=dev)
    store[:, :, :3] = -(1 << 30)
    tidx = store[:, :Hq, 3:3 + n]
    tidx.copy_(idx)
    g16 = [_strided(torch.full(t.shape, 7.0, dtype=t.dtype, device=dev), 8, 7.0) for t in (q, k, v)]
    tlse, tdelta = (torch.cat([t, torch.full((B, Hq, 3), float("nan"), device=dev)], -1)[:, :, :Sq] for t in (lse, delta))
    a = _C.UspBwdArgs()
    a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D, a.flags = B, Sq, Sk, Hq, Hkv, D, 0 if left is None else _C.USP_ATTN_WINDOW
    a.dq16, a.dk16, a.dv16 = (_C._t4(t) for t in g16)
    need = _C._feature_entry("usp_flash_bwd_gather_workspace_bytes")(a, n)
    assert need >= 2 * B * Hq * 128 * D * 4
    guarded = torch.full((need + 64,), 0x5a, dtype=torch.uint8, device=dev)
    _C.flash_bwd(tdo, tq, tk, tv, tlse, tdelta, None, None, None, D ** -0.5, True, dq16=g16[0], dk16=g16[1], dv16=g16[2],
                 window=None if left is None else (left, 0), key_index=tidx, key_index_ws=guarded[32:32 + need])
    _compare(g16, _reference(q, k, v, dout, idx, left), dt, "strided")
    assert (guarded[:32] == 0x5a).all() and (guarded[32 + need:] == 0x5a).all(), "a store left the workspace"
    for t, H in zip(g16, (Hq, Hkv, Hkv)):
        assert (t._base[:, 0] == 7).all() and (t._base[:, :, H] == 7).all() and (t._base[..., D:] == 7).all(), "a store left the view"


def test_more_items_than_cus_interleave_and_determinism():
    """4 x 33 x 256 / 128 = 264 dQ items: more than the CUs, so a workgroup's second pass reuses its LDS tiles and index ring.  Bit for
    bit against USP_LAUNCH_INTERLEAVE (one workgroup per item) and against a second plain run."""
    from yunchang_amd import _C
    from yunchang_amd.kernels import hip_attn_forward
    shape, dt, n, left = (4, 256, 256, 33, 3, 64), "bfloat16", 65, 31
    q, k, v = _inputs(*shape, dt)
    idx, dout = _lists(4, 33, n, 256, 9), _dout(q)
    out, lse = hip_attn_forward(q, k, v, softmax_scale=0.125, causal=True, window_size=(left, 0), key_index=idx)
    delta = (dout.float() * out.float()).sum(-1).permute(0, 2, 1).contiguous()
    runs = []
    for interleave in (False, True, False):
        g = [torch.empty_like(t) for t in (q, k, v)]
        _C.flash_bwd(dout, q, k, v, lse, delta, None, None, None, 0.125, True, dq16=g[0], dk16=g[1], dv16=g[2], window=(left, 0),
                     key_index=idx, interleave=interleave)
        runs.append(g)
    for other in runs[1:]:
        assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(runs[0], other))
    _compare(runs[0], _reference(q, k, v, dout, idx, left, 0.125), dt, "264 items")


def test_autograd_equals_the_explicit_backward_without_a_host_sync():
    from yunchang_amd.kernels import hip_attn_func
    shape, dt, n, left = SHAPES[0], "bfloat16", 65, 31
    q, k, v = _inputs(*shape, dt)
    idx, dout = _lists(shape[0], shape[3], n, shape[2], 100 + n), _dout(q)
    want = _backward(q, k, v, dout, idx, left)
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    torch.cuda.set_sync_debug_mode("error")
    try:
        hip_attn_func(*leaves, causal=True, window_size=(left, 0), key_index=idx).backward(dout)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(t.grad.view(torch.int16), w.view(torch.int16)) for t, w in zip(leaves, want))
