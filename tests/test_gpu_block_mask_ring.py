"""Block-sparse attention (block_mask=) across ring steps on the GPU: the basic ring of degree 2 and 4 on virtual ranks
(tests/virtual_grid.py), every (rank, step) launch under its strided view of ONE global mask, forward and backward against the
single-device call with the same global mask and against tests/block_mask_ref.py.  S_total = 1024, GQA 4/2, D 64, bf16, causal and
full.  Ulysses 2 and hybrid 2 x 1 / 2 x 2 on the virtual grid: the layer's own forward on every virtual rank, the gradients through
the layer's steps by hand.  The degree-1 layers (LongContextAttention with each ring, UlyssesAttention, the QKV-packed layer) run
through their public forward and autograd."""
import os

import pytest
import torch

import block_mask_ref as R
from golden_util import TOL, assert_close, grad_tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nccl_single():
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


def problem(dev, seed=17):
    B, S, Hq, Hkv, D = 1, 1024, 4, 2, 64
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv, Hq))
    mask = torch.rand(B, Hq, 8, 8, generator=g) < 0.5
    mask[:, :, 5, :] = False                      # a row block that sees nothing: empty on every rank that holds part of it
    mask |= torch.eye(8, dtype=torch.bool) & (torch.arange(8) != 5)[:, None]
    return q, k, v, do, mask.to(dev)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("P", [2, 4])
def test_basic_ring_on_virtual_ranks(dev, nccl_single, monkeypatch, P, causal):
    import yunchang_amd.ring.ring_flash_attn as RF
    from yunchang_amd.kernels.attention import hip_attn_backward, hip_attn_forward
    from yunchang_amd.ring.front_end import BlockMask
    from virtual_grid import VirtualGridPairwise, patch_dist, run_grid
    q, k, v, do, mask = problem(dev)
    S, D = q.shape[1], q.shape[3]
    rows, scale = S // P, D ** -0.5
    grid = VirtualGridPairwise(1, P, nccl_single)
    patch_dist(monkeypatch, grid)
    loc = [[t[:, r * rows:(r + 1) * rows].contiguous() for t in (q, k, v, do)] for r in range(P)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(P)]
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        _, rpg = grid.groups_of(r)
        lq, lk, lv, ldo = loc[r]
        with torch.cuda.stream(streams[r]):
            out, lse = RF.ring_flash_attn_forward(rpg, lq, lk, lv, scale, causal=causal, cu_doclens=BlockMask(mask))
            return [out, lse] + list(RF.ring_flash_attn_backward(rpg, ldo, lq, lk, lv, out, lse, scale, causal=causal,
                                                                 cu_doclens=BlockMask(mask)))
    res = run_grid(grid, P, rank_fn)
    torch.cuda.synchronize()
    ref = R.ref_all(do, q, k, v, scale, mask, causal)
    one = list(hip_attn_forward(q, k, v, causal=causal, block_mask=mask))
    g1 = [torch.empty_like(t) for t in (q, k, v)]
    hip_attn_backward(do, q, k, v, one[0], one[1], *g1, bwd_causal=causal, block_mask=mask)
    tol_o, tol_g = TOL["bfloat16"]["out"], grad_tol("bfloat16", 2)
    for r in range(P):
        sl = slice(r * rows, (r + 1) * rows)
        out, lse, dq, dk, dv = res[r]
        assert_close(out, ref[0][:, sl], *tol_o, f"ring {P} rank {r} out")
        assert_close(lse, ref[1][:, :, sl], 2e-3, 1e-4, f"ring {P} rank {r} lse")
        for got, want, single, name in ((dq, ref[2], g1[0], "dq"), (dk, ref[3], g1[1], "dk"), (dv, ref[4], g1[2], "dv")):
            assert_close(got, want[:, sl], *tol_g, f"ring {P} rank {r} {name}")
            assert_close(got, single[:, sl].double(), 2 * tol_g[0], 2 * tol_g[1], f"ring {P} rank {r} {name} vs one device")
        assert_close(out, one[0][:, sl].double(), 2 * tol_o[0], 2 * tol_o[1], f"ring {P} rank {r} out vs one device")


@pytest.mark.parametrize("layer", ["basic", "zigzag", "strip", "ulysses", "qkvpacked"])
def test_layers_at_degree_one(dev, nccl_single, layer):
    """The public layers on a 1-rank grid: the mask goes through the layer, the ring front end and the one-block call."""
    import yunchang_amd as Y
    q, k, v, do, mask = problem(dev, seed=23)
    Y.set_seq_parallel_pg(1, 1, 0, 1)
    if layer == "qkvpacked":
        k, v = (t.repeat_interleave(2, dim=2) for t in (k, v))
        qkv = torch.stack([q, k, v], dim=2).requires_grad_(True)
        out = Y.LongContextAttentionQKVPacked(ring_impl_type="basic", attn_type=Y.AttnType.HIP)(qkv, causal=True, block_mask=mask)
        out.backward(do)
        grads = [qkv.grad[:, :, i] for i in range(3)]
        G = 1
    else:
        tq, tk, tv = (t.clone().requires_grad_(True) for t in (q, k, v))
        if layer == "ulysses":
            import torch.distributed as dist
            attn = Y.UlyssesAttention(dist.group.WORLD, attn_type=Y.AttnType.HIP)
        else:
            attn = Y.LongContextAttention(ring_impl_type=layer, attn_type=Y.AttnType.HIP)
        out = attn(tq, tk, tv, causal=True, block_mask=mask)
        out.backward(do)
        grads = [tq.grad, tk.grad, tv.grad]
        G = 2
    ref = R.ref_all(do, q, k, v, q.shape[3] ** -0.5, mask, True)
    assert_close(out, ref[0], *TOL["bfloat16"]["out"], f"{layer} out")
    for g, r, name in zip(grads, ref[2:], ("dq", "dk", "dv")):
        assert_close(g, r, *grad_tol("bfloat16", G), f"{layer} {name}")


# ---- Ulysses 2 and hybrid 2 x 2 on the virtual grid -----------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("ud,rd,kind", [(2, 1, "ulysses"), (2, 1, "hybrid"), (2, 2, "hybrid")], ids=["ulysses2", "hybrid2x1", "hybrid2x2"])
def test_ulysses_and_hybrid_on_virtual_grid(dev, nccl_single, monkeypatch, ud, rd, kind, causal):
    """The head cut of the mask (P > 1) and, at 2 x 2, the head cut together with the ring's views of the global mask.  Forward:
    the layer's own forward on every virtual rank (three exchanges, the ring front end).  Gradients: the layer's steps by hand
    -- the same exchanges, the mask as the layer's own head options cut it, the ring backward -- because autograd keeps one
    worker thread per device, on which virtual ranks cannot wait for each other.  Both against the single-device call and the
    fp64 reference with the same global mask."""
    import yunchang_amd as Y
    import yunchang_amd.hybrid.attn_layer as HL
    import yunchang_amd.ring.front_end as FE
    import yunchang_amd.ring.ring_flash_attn as RF
    import yunchang_amd.ulysses.attn_layer as UL
    from yunchang_amd.comm.all_to_all import SeqAllToAll4D, SeqAllToAll4DKV
    from yunchang_amd.kernels.attention import hip_attn_backward, hip_attn_forward
    from virtual_grid import Ctx, VirtualGrid, patch_dist, run_grid
    q, k, v, do, mask = problem(dev, seed=31)
    S, Hq, D = q.shape[1], q.shape[2], q.shape[3]
    ws, scale = ud * rd, D ** -0.5
    rows = S // ws
    grid = VirtualGrid(ud, rd, nccl_single)
    patch_dist(monkeypatch, grid)
    for mod in (HL, FE, UL):
        monkeypatch.setattr(mod, "dist", grid)
    monkeypatch.setenv("USP_PIPELINE_ULYSSES", "0")
    Y.set_seq_parallel_pg(1, 1, 0, 1)
    layers = []
    for r in range(ws):
        upg, rpg = grid.groups_of(r)
        if kind == "ulysses":
            layers.append(Y.UlyssesAttention(upg, attn_type=Y.AttnType.HIP))
        else:
            lay = Y.LongContextAttention(ring_impl_type="basic", attn_type=Y.AttnType.HIP)
            lay.ulysses_pg, lay.ring_pg = upg, rpg
            layers.append(lay)
    loc = [[t[:, r * rows:(r + 1) * rows].contiguous() for t in (q, k, v, do)] for r in range(ws)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(ws)]
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        upg, rpg = grid.groups_of(r)
        lq, lk, lv, ldo = loc[r]
        to_heads = lambda t, fn=SeqAllToAll4D: fn.forward(Ctx(), upg, t, 2, 1, False, False)
        to_seq = lambda t: SeqAllToAll4D.forward(Ctx(), upg, t, 1, 2, False, False)
        with torch.cuda.stream(streams[r]), torch.no_grad():
            out = layers[r](lq, lk, lv, causal=causal, block_mask=mask)
            local = HL.local_options(None, 0.0, None, None, Hq, ud, grid.get_rank(upg), True, "", block_mask=mask)[0]["block_mask"]
            assert tuple(local.shape) == (1, Hq // ud, 8, 8)
            q2, k2, v2, do2 = to_heads(lq), to_heads(lk, SeqAllToAll4DKV), to_heads(lv, SeqAllToAll4DKV), to_heads(ldo)
            o2, lse = RF.ring_flash_attn_forward(rpg, q2, k2, v2, scale, causal=causal, cu_doclens=FE.BlockMask(local))
            g2 = RF.ring_flash_attn_backward(rpg, do2, q2, k2, v2, o2, lse, scale, causal=causal, cu_doclens=FE.BlockMask(local))
            return [out, to_seq(o2)] + [to_seq(g.contiguous()) for g in g2[:3]]
    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    ref = R.ref_all(do, q, k, v, scale, mask, causal)
    one = list(hip_attn_forward(q, k, v, causal=causal, block_mask=mask))
    g1 = [torch.empty_like(t) for t in (q, k, v)]
    hip_attn_backward(do, q, k, v, one[0], one[1], *g1, bwd_causal=causal, block_mask=mask)
    tol_o, tol_g = TOL["bfloat16"]["out"], grad_tol("bfloat16", 2)
    for r in range(ws):
        sl = slice(r * rows, (r + 1) * rows)
        out, out_hand, dq, dk, dv = res[r]
        assert torch.equal(out, out_hand), f"rank {r}: the layer's forward and its steps by hand"
        assert_close(out, ref[0][:, sl], *tol_o, f"{kind} {ud}x{rd} rank {r} out")
        assert_close(out, one[0][:, sl].double(), 2 * tol_o[0], 2 * tol_o[1], f"{kind} {ud}x{rd} rank {r} out vs one device")
        for got, want, single, name in ((dq, ref[2], g1[0], "dq"), (dk, ref[3], g1[1], "dk"), (dv, ref[4], g1[2], "dv")):
            assert_close(got, want[:, sl], *tol_g, f"{kind} {ud}x{rd} rank {r} {name}")
            assert_close(got, single[:, sl].double(), 2 * tol_g[0], 2 * tol_g[1], f"{kind} {ud}x{rd} rank {r} {name} vs one device")
