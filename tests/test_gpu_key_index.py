"""The gathered-key forward (csrc/usp_flash_fwd_gather.hip; include/usp_hip.h: USP_ATTN_KEY_INDEX) on the GPU, every element of out
and lse against fp64 attention under the mask of tests/key_index_ref.py.  An item is 128 query rows, a tile 64 list entries or keys."""
import pytest
import torch

import key_index_ref as R
from golden_util import TOL, assert_close

pytestmark = pytest.mark.gpu
LSE_TOL = (2e-3, 1e-4)
dev = torch.device("cuda:0")
_IN = {}


def _inputs(B, Sq, Sk, Hq, Hkv, D, dt):
    key = (B, Sq, Sk, Hq, Hkv, D, dt)
    if key not in _IN:
        gen = torch.Generator().manual_seed(len(_IN) + 1)
        _IN[key] = tuple(torch.randn(B, s, h, D, generator=gen).to(getattr(torch, dt)).to(dev) for s, h in ((Sq, Hq), (Sk, Hkv), (Sk, Hkv)))
    return _IN[key]


def _lists(B, Hq, n, Sk, seed):
    """Sorted distinct samples of [0, Sk), another one per (batch, head), padded with absent entries (>= Sk) where n > Sk.  Flat head 1
    is absent from the middle on, flat head 2 altogether, flat head 3 starts with a negative (absent) entry."""
    gen = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.cat([torch.randperm(Sk, generator=gen)[:n].sort().values, torch.arange(Sk, Sk + max(0, n - Sk))])
                       for _ in range(B * Hq)])
    idx[1, n // 2:] = Sk + 7
    idx[2] = torch.arange(Sk, Sk + n)
    if B * Hq > 3 and n > 1:
        idx[3, 0] = -5
    return idx.view(B, Hq, n).to(torch.int32).to(dev)


def _check(out, lse, q, k, v, idx, left, dt, what):
    ro, rl = R.attention(q, k, v, q.shape[-1] ** -0.5, R.mask(q.shape[1], k.shape[1], idx, left))
    assert_close(out, ro, *TOL[dt]["out"], f"{what} out")
    assert_close(lse, rl, *LSE_TOL, f"{what} lse")


@pytest.mark.parametrize("left", [None, 0, 31, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("shape", [(1, 320, 320, 4, 1, 128), (2, 192, 192, 2, 2, 64), (1, 77, 333, 3, 1, 128)], ids=str)
def test_forward_against_fp64(shape, dt, n, left):
    """Entries inside the band count once, entries above an early row's diagonal are masked, and without a window the rows before a
    head's first listed key see nothing (out = 0, lse = -inf)."""
    from yunchang_amd import _C
    from yunchang_amd.kernels import hip_attn_forward
    B, Sq, Sk, Hq, Hkv, D = shape
    q, k, v = _inputs(*shape, dt)
    idx = _lists(B, Hq, n, Sk, 100 + n)
    out, lse = hip_attn_forward(q, k, v, causal=True, window_size=(-1, -1) if left is None else (left, 0), key_index=idx)
    assert _C.last_launch_kinds() == ("fwd_gather",)
    _check(out, lse, q, k, v, idx, left, dt, f"{shape} {dt} n={n} left={left}")
    if left is None:
        b, h = divmod(2, Hq)
        assert torch.isinf(lse[b, h]).all() and (out[b, :, h] == 0).all(), "the all-absent head saw a key"


def test_needle_is_exact_for_every_key_of_two_tiles_plus_one():
    """No window, one listed key per head: every row at or past it returns that key's v bit for bit (p = 1, l = 1), every row before
    it zero -- a gathered row that lands in another LDS row or slot, or is paired with another column's mask, puts other bits there."""
    from yunchang_amd.kernels import hip_attn_forward
    B, S, Hq, G, D = 1, 160, 2, 2, 64
    q, k, v = _inputs(B, S, S, Hq, Hq // G, D, "bfloat16")
    rows = torch.arange(S, device=dev)
    for key in range(129):
        keys = torch.tensor([key, (key + 64) % 129], device=dev)
        out, lse = hip_attn_forward(q, k, v, causal=True, key_index=keys.to(torch.int32)[:, None])
        past = rows[:, None] >= keys[None, :]                                        # (S, Hq)
        want = torch.where(past[None, :, :, None], v[:, keys, 0][:, None].expand(B, S, Hq, D), torch.zeros((), dtype=v.dtype, device=dev))
        assert torch.equal(out.view(torch.int16), want.contiguous().view(torch.int16)), f"key {key}"
        assert torch.equal(torch.isinf(lse[0]).T, ~past), f"key {key}: lse"


def _strided(t, pad, fill):
    """`t` as a view with padded row, head and batch strides inside `fill`-ed storage"""
    B, S, H, W = t.shape
    buf = torch.full((B, S + 1, H + 1, W + pad), fill, dtype=t.dtype, device=dev)
    view = buf[:, 1:, :H, :W]
    view.copy_(t)
    return view


@pytest.mark.parametrize("left", [None, 31])
def test_strided_operands_and_list_in_poisoned_memory(left):
    from yunchang_amd import _C
    shape, dt, n = (2, 192, 192, 2, 2, 64), "bfloat16", 65
    B, Sq, Sk, Hq, Hkv, D = shape
    q, k, v = _inputs(*shape, dt)
    tq, tk, tv = (_strided(t, 8, float("nan")) for t in (q, k, v))
    idx = _lists(B, Hq, n, Sk, 5)
    store = torch.full((B, Hq + 1, n + 9), 0x40000000, dtype=torch.int32, device=dev)
    store[:, :, :3] = -(1 << 30)
    tidx = store[:, :Hq, 3:3 + n]
    tidx.copy_(idx)
    out = _strided(torch.full(q.shape, 7.0, dtype=q.dtype, device=dev), 8, 7.0)
    lse = torch.full((B, Hq, Sq + 3), 7.0, device=dev)[:, :, :Sq]
    _C.flash_fwd(tq, tk, tv, D ** -0.5, True, lse, out=out, window=None if left is None else (left, 0), key_index=tidx)
    _check(out, lse, q, k, v, idx, left, dt, "strided")
    assert (out._base[:, 0] == 7).all() and (out._base[:, :, Hq] == 7).all() and (out._base[..., D:] == 7).all(), "a store left the view"


@pytest.mark.parametrize("S", [256, 512])
def test_more_items_than_cus_and_interleave(S):
    """4 x 33 x S / 128 = 264 | 528 items: more than the CUs, and (two workgroups per CU) more than the resident workgroups, whose
    second pass reuses LDS tiles, index ring and row statistics.  Bit for bit against USP_LAUNCH_INTERLEAVE (one workgroup per item)."""
    from yunchang_amd import _C
    shape, dt, n, left = (4, S, S, 33, 3, 64), "bfloat16", 65, 31
    q, k, v = _inputs(*shape, dt)
    idx = _lists(4, 33, n, S, 9)
    got = []
    for interleave in (False, True):
        out, lse = torch.empty_like(q), torch.empty(4, 33, S, device=dev)
        _C.flash_fwd(q, k, v, 0.125, True, lse, out=out, window=(left, 0), key_index=idx, interleave=interleave)
        assert _C.last_launch_kinds() == ("fwd_gather",)
        got.append((out, lse))
    assert torch.equal(got[0][0].view(torch.int16), got[1][0].view(torch.int16)) and torch.equal(got[0][1], got[1][1])
    _check(*got[0], q, k, v, idx, left, dt, f"{4 * 33 * S // 128} items")
