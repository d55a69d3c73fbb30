"""Block-sparse attention (block_mask=) on the GPU: the block-sparse instantiations of the two-waves-per-SIMD kernels
(usp_flash_fwd_bsp / usp_flash_bwd_bsp) and their list builder against tests/block_mask_ref.py (fp64, on the device, the mask
expanded from its definition alone).  Every element is compared, at the project's tolerances (golden_util.TOL, grad_tol) and the
lse bound of tests/test_gpu_doc_mask.py.

Shapes (B, S, Hq, Hkv, D): (1, 640, 4, 2, 128) -- five row blocks, so the last 256-row dQ block holds one; (2, 384, 2, 2, 64);
(1, 333, 3, 1, 32) -- a ragged last block and three query heads in one dK/dV item; (1, 128, 1, 1, 128) -- a single block.
Masks: all set; the diagonal; seeded random at about half density per head and batch entry; random with one row block and one key
block all false (rows that see nothing, keys nobody sees); lower-triangular with every bit above the diagonal SET under causal,
which must be ignored; one whose two row blocks of a 256-row dQ block differ in every column (every dQ entry is live for exactly
one half)."""
import numpy as np
import pytest
import torch

import block_mask_ref as R
from golden_util import TOL, assert_close, grad_tol, make_inputs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 640, 4, 2, 128), (2, 384, 2, 2, 64), (1, 333, 3, 1, 32), (1, 128, 1, 1, 128)]
MASKS = ("all", "diag", "random", "holes", "tril", "halves")
LSE_TOL = (2e-3, 1e-4)


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def make_mask(kind, B, Hq, S, causal, seed=0):
    """(the mask handed to the kernels, the mask the reference takes), torch.bool (B, Hq, nb, nb) on the host."""
    nb = R.n_blocks(S)
    g = torch.Generator().manual_seed(1000 * seed + 7 * S + Hq)
    eye = torch.eye(nb, dtype=torch.bool).expand(B, Hq, nb, nb)
    if kind == "all":
        m = torch.ones(B, Hq, nb, nb, dtype=torch.bool)
    elif kind == "diag":
        m = eye.clone()
    elif kind == "random":
        m = torch.rand(B, Hq, nb, nb, generator=g) < 0.5
    elif kind == "holes":
        m = torch.rand(B, Hq, nb, nb, generator=g) < 0.6
        m[:, :, nb // 2, :] = False
        m[:, :, :, nb // 3] = False
    elif kind == "tril":
        low = torch.tril(torch.rand(B, Hq, nb, nb, generator=g) < 0.6) | eye
        if causal:          # every bit above the diagonal set: ignored under causal
            return low | torch.triu(torch.ones(nb, nb, dtype=torch.bool), 1), low
        m = low
    else:                   # halves: row blocks 2i and 2i + 1 are each other's complement
        a = torch.rand(B, Hq, (nb + 1) // 2, nb, generator=g) < 0.5
        m = torch.stack([a, ~a], dim=3).reshape(B, Hq, -1, nb)[:, :, :nb].contiguous()
    return m, m


_IN = {}


def inputs(dev, B, S, Hq, Hkv, D, dt):
    key = (B, S, Hq, Hkv, D, dt)
    if key not in _IN:
        _IN[key] = [torch.from_numpy(x).to(getattr(torch, dt)).to(dev) for x in make_inputs(B, S, Hq, Hkv, D, seed=S + D)]
    return _IN[key]          # q, k, v, dout


def run_block(q, k, v, do, mask, causal, **kw):
    from yunchang_amd.kernels.attention import hip_attn_backward, hip_attn_forward
    out, lse = hip_attn_forward(q, k, v, causal=causal, block_mask=mask, **kw)
    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
    hip_attn_backward(do, q, k, v, out, lse, dq, dk, dv, bwd_causal=causal, block_mask=mask, **kw)
    return out, lse, dq, dk, dv


def check(got, ref, dt, G, what):
    out, lse, dq, dk, dv = got
    assert_close(out, ref[0], *TOL[dt]["out"], f"{what} out")
    assert_close(lse, ref[1], *LSE_TOL, f"{what} lse")
    for g, r, name in zip((dq, dk, dv), ref[2:], ("dq", "dk", "dv")):
        assert_close(g, r, *grad_tol(dt, G), f"{what} {name}")


# ---- 1. block launches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-S%d-H%d/%d-D%d" % s)
def test_block_launches(dev, shape, dt, causal, kind):
    B, S, Hq, Hkv, D = shape
    q, k, v, do = inputs(dev, B, S, Hq, Hkv, D, dt)
    given, meant = make_mask(kind, B, Hq, S, causal)
    ref = R.ref_all(do, q, k, v, D ** -0.5, meant.to(dev), causal)
    got = run_block(q, k, v, do, given.to(dev), causal)
    check(got, ref, dt, Hq // Hkv, f"{shape} {dt} causal={causal} {kind}")
    if kind == "holes":      # rows that see nothing: exactly 0 / -inf, and zero gradients
        dead = torch.isinf(ref[1])
        if not causal:
            assert bool(dead.any())
        assert bool((got[1][dead] == float("-inf")).all())
        assert bool((got[0].transpose(1, 2)[dead] == 0).all()) and bool((got[2].transpose(1, 2)[dead] == 0).all())


def test_fails_without_the_feature(dev):
    """The keyword itself: on a package without block_mask this is a TypeError (unexpected keyword)."""
    from yunchang_amd.kernels.attention import hip_attn_forward
    q, k, v, _ = inputs(dev, 1, 128, 1, 1, 128, "bfloat16")
    out, lse = hip_attn_forward(q, k, v, causal=True, block_mask=torch.ones(1, 1, dtype=torch.bool, device=dev))
    ref = R.ref_fwd(q, k, v, 128 ** -0.5, torch.ones(1, 1, dtype=torch.bool), True)
    assert_close(out, ref[0], *TOL["bfloat16"]["out"], "out")


@pytest.mark.parametrize("form", ["2d", "3d", "strided", "last-dim-strided"])
def test_mask_forms_and_strides(dev, form):
    """(nb, nb) and (Hq, nb, nb) broadcast; a strided, non-contiguous view gives the bits of its contiguous copy."""
    B, S, Hq, Hkv, D = 2, 384, 2, 2, 64
    q, k, v, do = inputs(dev, B, S, Hq, Hkv, D, "bfloat16")
    nb = R.n_blocks(S)
    g = torch.Generator().manual_seed(3)
    if form == "2d":
        view = (torch.rand(nb, nb, generator=g) < 0.6).to(dev)
    elif form == "3d":
        view = (torch.rand(Hq, nb, nb, generator=g) < 0.6).to(dev)
    elif form == "strided":          # a window of a bigger mask: row stride 2 nb + 1, odd batch and head strides
        big = (torch.rand(B, Hq + 1, 2 * nb, 2 * nb + 1, generator=g) < 0.6).to(dev)
        view = big[:, 1:, nb:, 1:nb + 1]
        assert not view.is_contiguous() and view.stride(-1) == 1
    else:                            # last dimension strided: made contiguous once
        big = (torch.rand(B, Hq, nb, 2 * nb, generator=g) < 0.6).to(dev)
        view = big[..., ::2]
        assert view.stride(-1) == 2
    dense = R.mask4(view, B, Hq, S).contiguous()
    a = run_block(q, k, v, do, view, True)
    b = run_block(q, k, v, do, dense, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    check(a, R.ref_all(do, q, k, v, D ** -0.5, dense, True), "bfloat16", 1, form)


def test_padded_head_dim_and_autograd(dev):
    """hip_attn_func with a (B, Hq, nb, nb) mask at head dim 96 (zero-padded to 128): forward and autograd gradients."""
    from yunchang_amd.kernels.attention import hip_attn_func
    B, S, Hq, Hkv, D = 2, 384, 4, 2, 96
    q, k, v, do = (t.clone() for t in inputs(dev, B, S, Hq, Hkv, D, "bfloat16"))
    mask = make_mask("random", B, Hq, S, True, seed=5)[0].to(dev)
    for t in (q, k, v):
        t.requires_grad_(True)
    out, lse, _ = hip_attn_func(q, k, v, causal=True, return_attn_probs=True, block_mask=mask)
    out.backward(do)
    ref = R.ref_all(do, q.detach(), k.detach(), v.detach(), D ** -0.5, mask, True)
    check((out.detach(), lse, q.grad, k.grad, v.grad), ref, "bfloat16", 2, "hip_attn_func D96")


def test_no_host_sync(dev):
    """Nothing on the call path reads a device value on the host: forward and backward under sync debug mode "error"."""
    from yunchang_amd.kernels.attention import hip_attn_func
    B, S, Hq, Hkv, D = 1, 640, 4, 2, 128
    q, k, v, do = (t.clone().requires_grad_(True) for t in inputs(dev, B, S, Hq, Hkv, D, "bfloat16"))
    mask = make_mask("random", B, Hq, S, True)[0].to(dev)
    hip_attn_func(q, k, v, causal=True, block_mask=mask).backward(do.detach())       # (first call: library load, caches)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for t in (q, k, v):
            t.grad = None
        gate = torch.rand(B, Hq, 5, 5, device=dev) < 0.7      # the mask as the output of a kernel on the same stream
        hip_attn_func(q, k, v, causal=True, block_mask=gate).backward(do.detach())
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(q.grad.float()).all())


# ---- 2. the built lists ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("shape", [(1, 640, 4, 2, 128), (2, 384, 2, 2, 64), (1, 333, 3, 1, 32), (1, 128, 1, 1, 128), (1, 8300, 1, 1, 32),
                                   (1, 300, 3, 1, 32), (1, 4400, 1, 1, 32)],
                         ids=lambda s: "B%d-S%d-H%d" % s[:3])
def test_built_lists(dev, shape, causal, kind):
    """Counts, order, the causal drop, the half bits and the transpose, read back and compared with a numpy enumeration.
    S = 8300: 65 blocks, more than one 64-lane step of the builder; its last block holds 108 keys, so both of its tiles exist
    (tiles 128 and 129 of 130).  S = 300 and S = 4400 (44 and 48 keys in the last block): a last block whose second tile does not
    exist."""
    from yunchang_amd import _C
    B, S, Hq, Hkv, D = shape
    q, k, v, do = inputs(dev, B, S, Hq, Hkv, D, "bfloat16")
    mask = make_mask(kind, B, Hq, S, causal)[0]
    nb = R.n_blocks(S)
    lay = _C.block_list_layout(B, Hq, nb)
    assert _C.block_list_bytes(B, Hq, nb) == 4 * lay["ints"]
    lists = torch.full((lay["ints"],), -7, dtype=torch.int32, device=dev)
    out = torch.empty_like(q)
    lse = torch.empty((B, Hq, S), dtype=torch.float32, device=dev)
    _C.flash_fwd(q, k, v, D ** -0.5, causal, lse, out=out, bsp=mask.to(dev), bsp_lists=lists)
    delta = torch.zeros_like(lse)
    dq, dk, dv = (torch.empty(t.shape, dtype=torch.float32, device=dev) for t in (q, k, v))
    _C.flash_bwd(do, q, k, v, lse, delta, dq, dk, dv, D ** -0.5, causal, bsp=mask.to(dev), bsp_lists=lists)
    got = lists.cpu().numpy()
    want = R.enumerate_lists(mask.numpy(), S, causal)
    for fam in ("fwd", "dq", "dkdv"):
        off, per, stride = lay[fam]
        for (b, h, i), ent in want[fam].items():
            base = off + ((b * Hq + h) * per + i) * stride
            assert got[base] == len(ent), (fam, b, h, i, got[base], len(ent))
            assert list(got[base + 1:base + 1 + len(ent)]) == ent, (fam, b, h, i)


# ---- 3. an all-set mask gives the bits of the plain two-waves-per-SIMD launch of the same workgroup shape ------------------------
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("shape,dt", [((1, 640, 4, 2, 128), "bfloat16"), ((2, 384, 2, 2, 64), "float16"), ((1, 333, 3, 1, 32), "bfloat16")],
                         ids=lambda s: str(s))
def test_all_set_mask_is_the_plain_launch(dev, shape, dt, causal):
    """Forward: these shapes have fewer than 256 eight-wave items, so the plain wave32 launch is the 4-wave one, like the
    block-sparse launch.  dQ and dK/dV have one shape each.  Cuts off on both sides (the mask is served uncut)."""
    from yunchang_amd import _C
    B, S, Hq, Hkv, D = shape
    q, k, v, do = inputs(dev, B, S, Hq, Hkv, D, dt)
    mask = torch.ones(R.n_blocks(S), R.n_blocks(S), dtype=torch.bool, device=dev)
    res = []
    for kw in (dict(family="wave32"), dict(bsp=mask)):
        out = torch.full_like(q, float("nan"))
        lse = torch.full((B, Hq, S), float("nan"), dtype=torch.float32, device=dev)
        _C.flash_fwd(q, k, v, D ** -0.5, causal, lse, out=out, k_splits=0, **kw)
        kinds = _C.last_launch_kinds()
        assert kinds == ("fwd_wave4",), kinds
        delta = torch.empty_like(lse)
        _C.bwd_delta(do, out, delta)
        dq, dk, dv = (torch.full(t.shape, float("nan"), dtype=torch.float32, device=dev) for t in (q, k, v))
        _C.flash_bwd(do, q, k, v, lse, delta, dq, dk, dv, D ** -0.5, causal, splits=(0, 0), dkdv_heads=Hq // Hkv, **kw)
        assert {"dkdv_wave8", "dq_wave8"} <= set(_C.last_launch_kinds())
        res.append((out, lse, dq, dk, dv))
    for name, a, b in zip(("out", "lse", "dq", "dk", "dv"), *res):
        assert torch.equal(a, b), name


# ---- 4. persistent launch depth: more work items than resident workgroups ---------------------------------------------------------
def test_persistent_launch_depth(dev):
    """B2 H16/16 S2176 D32: 544 forward items on 512 slots, 544 dK/dV and 288 dQ items on 256: every element against the
    reference, and the persistent launch bit for bit equal to USP_LAUNCH_INTERLEAVE (one workgroup per item)."""
    from yunchang_amd import _C
    B, S, Hq, Hkv, D = 2, 2176, 16, 16, 32
    q, k, v, do = inputs(dev, B, S, Hq, Hkv, D, "bfloat16")
    mask = make_mask("random", B, Hq, S, True, seed=11)[0].to(dev)
    ref = R.ref_all(do, q, k, v, D ** -0.5, mask, True)
    res = []
    for interleave in (False, True):
        out = torch.full_like(q, float("nan"))
        lse = torch.full((B, Hq, S), float("nan"), dtype=torch.float32, device=dev)
        _C.flash_fwd(q, k, v, D ** -0.5, True, lse, out=out, bsp=mask, interleave=interleave)
        delta = torch.empty_like(lse)
        _C.bwd_delta(do, out, delta)
        dq, dk, dv = (torch.full(t.shape, float("nan"), dtype=torch.float32, device=dev) for t in (q, k, v))
        _C.flash_bwd(do, q, k, v, lse, delta, dq, dk, dv, D ** -0.5, True, bsp=mask, interleave=interleave)
        res.append((out, lse, dq, dk, dv))
    check(res[0], ref, "bfloat16", 1, "persistent")
    for name, a, b in zip(("out", "lse", "dq", "dk", "dv"), *res):
        assert torch.equal(a, b), name


# ---- 5. merge_in / acc / final_begin: two launches over the two key halves equal one over all keys ---------------------------------
@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
def test_merge_in_over_key_halves(dev, dt):
    """The mask restricted to the key blocks [0, 3) and then to [3, 5), the second launch with merge_in on the first one's
    (acc, lse) and every row final: equal to one launch within the tolerance; row block 1 sees nothing in the second half and
    row block 3 nothing in the first, row block 2 nothing at all."""
    from yunchang_amd import _C
    B, S, Hq, Hkv, D = 1, 640, 4, 2, 128
    q, k, v, _ = inputs(dev, B, S, Hq, Hkv, D, dt)
    mask = make_mask("random", B, Hq, S, False, seed=2)[0]
    mask[:, :, 1, 3:] = False
    mask[:, :, 3, :3] = False
    mask[:, :, 2, :] = False
    first, second = mask.clone(), mask.clone()
    first[..., 3:] = False
    second[..., :3] = False
    out = torch.full_like(q, float("nan"))
    acc = torch.full(q.shape, float("nan"), dtype=torch.float32, device=dev)
    lse = torch.full((B, Hq, S), float("nan"), dtype=torch.float32, device=dev)
    _C.flash_fwd(q, k, v, D ** -0.5, False, lse, out=out, acc=acc, final_begin=0, final_end=0, bsp=first.to(dev))
    _C.flash_fwd(q, k, v, D ** -0.5, False, lse, out=out, acc=acc, merge_in=True, bsp=second.to(dev))
    ref = R.ref_fwd(q, k, v, D ** -0.5, mask.to(dev), False)
    assert_close(out, ref[0], *TOL[dt]["out"], "merged out")
    assert_close(lse, ref[1], *LSE_TOL, "merged lse")
    assert bool(torch.isinf(ref[1][:, :, 256:384]).all())


# ---- 6. the C ABI's refusals -----------------------------------------------------------------------------------------------------
def test_abi_refusals(dev):
    import ctypes
    from yunchang_amd import _C
    q, k, v, _ = inputs(dev, 1, 640, 4, 2, 128, "bfloat16")
    lse = torch.zeros((1, 4, 640), dtype=torch.float32, device=dev)
    out = torch.zeros_like(q)
    mask = torch.ones(5, 5, dtype=torch.bool, device=dev).view(torch.uint8)
    lists = torch.zeros(_C.block_list_bytes(1, 4, 5), dtype=torch.uint8, device=dev)
    fn = _C._feature_entry("usp_flash_fwd_bsp")
    assert _C.load().usp_attn_features() & _C.USP_ATTN_BLOCK_MASK

    def call(a, m=mask, strides=(0, 0, 5), ls=lists):
        return fn(ctypes.byref(a), _C._ptr(m), *strides, _C._ptr(ls), _C._stream())
    args = lambda **kw: _C._fwd_args(q, k, v, 128 ** -0.5, True, lse, out, None, False, 0, None, False, 0, **kw)
    assert call(args()) == 0
    assert call(args(), strides=(0, -1, 5)) == -1
    assert call(args(), ls=None) == -1
    for kw in (dict(window=(64, 0)), dict(shift=128), dict(softcap=30.0), dict(family_flag=_C.USP_FORCE_ROW64)):
        out.fill_(7.0)
        assert call(args(**kw)) == -2, kw
        assert bool((out == 7.0).all())                         # nothing launched or written
    a = _C._fwd_args(q, k[:, :512], v[:, :512], 128 ** -0.5, False, lse, out, None, False, 0, None, False, 0)
    assert call(a) == -2                        # Sq != Sk
    torch.cuda.synchronize()
