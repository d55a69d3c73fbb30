"""The antidiagonal block gate on the GPU: the weights against the fp64 reference under the derived bound of tests/block_antidiag_ref.py,
the selector bit for bit on planted dyadic weights, block_select= == block_mask= on one device and through Ulysses 2, repeatability."""
import pytest
import torch

import block_antidiag_ref as AD
from test_gpu_block_select import dev, gather_grid, guarded, nccl_single, ring_problem, strided  # noqa: F401

pytestmark = pytest.mark.gpu


def _qk(B, S, Hq, Hkv, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple((1.5 * torch.randn(B, S, h, D, generator=g)).to(dtype) for h in (Hq, Hkv))


# ---- 1. the weights against the fp64 reference ------------------------------------------------------------------------------------
# every S (one block; a one-row last block; no multiple of any stride; several items with a ragged end), stride, D, dtype, mask and
# head grouping, and each pairing the loops distinguish: heads side by side (4, 1), an idle wave and two head chunks (6, 2 -> G = 3;
# 8, 1), sub-row tiles side by side (2, 2 -> G = 1), the resident (stride 4 / 8) and the streamed (16) Q fragments at every D
CASES = [(128, 4, 32, torch.bfloat16, True, 4, 1), (128, 16, 128, torch.float16, False, 2, 2), (257, 8, 64, torch.bfloat16, True, 6, 2),
         (257, 4, 128, torch.float16, False, 4, 1), (300, 16, 32, torch.bfloat16, True, 2, 2), (300, 8, 128, torch.bfloat16, False, 6, 2),
         (1088, 4, 64, torch.float16, True, 2, 2), (1088, 8, 32, torch.float16, False, 4, 1), (1088, 16, 64, torch.bfloat16, False, 6, 2),
         (1088, 16, 128, torch.bfloat16, True, 4, 1), (1088, 8, 128, torch.float16, True, 2, 2), (1088, 4, 128, torch.bfloat16, True, 8, 1)]


@pytest.mark.parametrize("S,stride,D,dtype,causal,Hq,Hkv", CASES)
def test_weights_against_reference(dev, S, stride, D, dtype, causal, Hq, Hkv):
    import yunchang_amd as Y
    q, k = _qk(2, S, Hq, Hkv, D, dtype, S + stride + D)
    scale = D ** -0.5
    got = Y.antidiag_block_weights(q.to(dev), k.to(dev), causal=causal, stride=stride)
    AD.check(got, q, k, scale, causal, stride, f"S={S} s={stride} D={D} {dtype} causal={causal} H={Hq}/{Hkv}")
    assert not causal or float(got.triu(1).abs().max()) == 0.0


def test_weights_on_strided_views_between_guards(dev):
    """q and k as strided views in NaN-poisoned buffers, `out` a strided view between guard words."""
    from yunchang_amd import _C
    S, stride, Hq, Hkv, D, nb = 300, 8, 4, 2, 64, 3
    q, k = _qk(1, S, Hq, Hkv, D, torch.bfloat16, 5)
    raw, check = guarded((1, Hq + 1, nb + 1, (nb + 2) * 4), dev)
    buf = raw.view(torch.float32)
    view = buf[:, :Hq, :nb, 1:nb + 1]
    _C.block_antidiag_weights(strided(q, dev), strided(k, dev), D ** -0.5, True, stride, out=view)
    check()
    AD.check(view, q, k, D ** -0.5, True, stride, "strided")
    outside = buf.clone()
    outside[:, :Hq, :nb, 1:nb + 1] = float("nan")
    assert bool(outside.isnan().all()), "an element outside the view was written"      # (0xFFFFFFFF is a NaN)


def test_weights_with_more_items_than_resident_workgroups(dev):
    """A persistent launch whose workgroups walk several items each, every element checked (the reference in fp64 on the device).
    G = 4: an item is one sub-row tile of the four heads of a KV group, B * Hkv * ceil(S / stride / 32) = 2 * 8 * 64 = 1024 items."""
    import yunchang_amd as Y
    B, S, Hq, Hkv, D, stride = 2, 8192, 32, 8, 32, 4
    assert Hq // Hkv == 4 and B * Hkv * (S // stride // 32) > 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    q, k = (t.to(dev) for t in _qk(B, S, Hq, Hkv, D, torch.bfloat16, 9))
    got = Y.antidiag_block_weights(q, k, causal=True, stride=stride)
    for h in range(0, Hkv, 2):                                            # (two KV groups at a time: 0.5 GiB of sub-scores)
        AD.check(got[:, 4 * h:4 * h + 8], q[:, :, 4 * h:4 * h + 8], k[:, :, h:h + 2], D ** -0.5, True, stride, f"persistent, KV heads {h}, {h + 1}")


# ---- 2. selection from weights, bit for bit ---------------------------------------------------------------------------------------
def _planted(nbk, seed):
    """(1, 3, nbq, nbk) fp32, multiples of 2^-12 (every partial sum exact in fp32): head 0 distinct values in a shuffled order,
    head 1 runs of equal values (ties across any cut), head 2 almost all the weight on the row's own and the first block."""
    g = torch.Generator().manual_seed(seed)
    nbq = min(nbk, 6)
    rows = torch.arange(nbk - nbq, nbk)
    w = torch.zeros(1, 3, nbq, nbk)
    for i in range(nbq):
        w[0, 0, i] = (torch.randperm(nbk, generator=g) + 1).float()
        w[0, 1, i] = (torch.randint(1, 4, (nbk,), generator=g) * 8).float()
        w[0, 2, i] = 1.0
        w[0, 2, i, 0] = w[0, 2, i, rows[i]] = 4096.0
    return w * 2.0 ** -12, int(rows[0])


@pytest.mark.parametrize("nbk", [1, 63, 64, 65, 300])
def test_selection_from_planted_weights(dev, nbk):
    from yunchang_amd import _C
    w, row0 = _planted(nbk, nbk)
    # a strided view of the weights inside a larger buffer
    big = torch.full((1, 4, w.shape[2] + 1, nbk + 3), float("nan"), device=dev)
    view = big[:, :3, 1:, :nbk]
    view.copy_(w)
    for causal, top_p, kf, kl in ((False, 0.5, 0, 0), (True, 0.5, 0, 1), (False, 0.9, 1, 1), (True, 1.0, 0, 1), (False, 1.0, 2, 0), (True, 0.25, 1, 2)):
        got = _C.block_select_weights(view, top_p, causal, kf, kl, row0).cpu()
        want = AD.select_from_weights_ref(w, top_p, causal, kf, kl, row0)
        assert torch.equal(got, want), (nbk, causal, top_p, kf, kl, (got != want).nonzero()[:4].tolist())


# ---- 3. identities ----------------------------------------------------------------------------------------------------------------
def test_composition_and_block_select_keyword(dev):
    import yunchang_amd as Y
    from yunchang_amd.kernels.attention import hip_attn_func
    q, k, v, do = ring_problem(dev, 31)
    w = Y.antidiag_block_weights(q, k, causal=True, stride=8)
    mask = Y.select_blocks_antidiag(q, k, 0.7, causal=True, stride=8, keep_first=1)
    assert torch.equal(mask, Y.select_blocks_from_weights(w, 0.7, causal=True, keep_first=1))
    assert bool(mask.diagonal(dim1=-2, dim2=-1).all()) and int(mask.sum()) < mask.shape[0] * mask.shape[1] * 36, "something is cut"
    res = []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for kw in (dict(block_select=Y.BlockSelectAntidiag(0.7, 8, 1, 1)), dict(block_mask=mask)):
            tq, tk, tv = (t.clone().requires_grad_(True) for t in (q, k, v))
            out, lse, _ = hip_attn_func(tq, tk, tv, causal=True, return_attn_probs=True, **kw)
            out.backward(do)
            res.append((out.detach(), lse.detach(), tq.grad, tk.grad, tv.grad))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b, name in zip(res[0], res[1], ("out", "lse", "dq", "dk", "dv")):
        assert torch.equal(a, b), name


def test_ulysses_2_on_the_virtual_grid(dev, nccl_single, monkeypatch):
    import yunchang_amd as Y
    import yunchang_amd.hybrid.attn_layer as HL
    import yunchang_amd.ring.front_end as FE
    import yunchang_amd.ulysses.attn_layer as UL
    from yunchang_amd.comm.all_to_all import SeqAllToAll4D, SeqAllToAll4DKV, local_heads
    from yunchang_amd.kernels.attention import hip_attn_forward
    from golden_util import TOL, assert_close
    from virtual_grid import Ctx, patch_dist, run_grid
    q, k, v, _ = ring_problem(dev, 37)
    sel = Y.BlockSelectAntidiag(0.7, 16, 1, 1)
    grid = gather_grid(2, 1, nccl_single)
    patch_dist(monkeypatch, grid)
    for mod in (HL, FE, UL):
        monkeypatch.setattr(mod, "dist", grid)
    monkeypatch.setenv("USP_PIPELINE_ULYSSES", "0")
    Y.set_seq_parallel_pg(1, 1, 0, 1)
    layers = [Y.UlyssesAttention(grid.groups_of(r)[0], attn_type=Y.AttnType.HIP) for r in range(2)]
    loc = [[t[:, r * 512:(r + 1) * 512].contiguous() for t in (q, k, v)] for r in range(2)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        upg, rpg = grid.groups_of(r)
        with torch.cuda.stream(streams[r]), torch.no_grad():
            q2, k2 = (fn.forward(Ctx(), upg, t, 2, 1, False, False) for fn, t in ((SeqAllToAll4D, loc[r][0]), (SeqAllToAll4DKV, loc[r][1])))
            return layers[r](*loc[r], causal=True, block_select=sel), FE.select_block_rows(q2, k2, sel, 64 ** -0.5, True, rpg).mask
    res = run_grid(grid, 2, rank_fn)
    torch.cuda.synchronize()
    mask = Y.select_blocks_antidiag(q, k, 0.7, causal=True, stride=16, keep_first=1)
    one, tol = hip_attn_forward(q, k, v, causal=True, block_mask=mask)[0], TOL["bfloat16"]["out"]
    for r in range(2):
        assert torch.equal(res[r][1], mask[:, local_heads(4, 2, r)]), f"rank {r}: its heads of the single-device mask"
        assert_close(res[r][0], one[:, r * 512:(r + 1) * 512].double(), 2 * tol[0], 2 * tol[1], f"ulysses 2 rank {r} out vs one device")


# ---- 4. repeatability -------------------------------------------------------------------------------------------------------------
def test_weights_repeat_and_do_not_depend_on_the_batch(dev):
    import yunchang_amd as Y
    q, k = (t.to(dev) for t in _qk(3, 1088, 6, 2, 64, torch.bfloat16, 41))
    a = Y.antidiag_block_weights(q, k, causal=True, stride=8)
    assert torch.equal(a, Y.antidiag_block_weights(q, k, causal=True, stride=8))
    assert torch.equal(a[:1], Y.antidiag_block_weights(q[:1], k[:1], causal=True, stride=8))
