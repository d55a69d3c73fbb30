"""Top-k block selection (`block_select=`) on the GPU: usp_block_means against fp64 within the derived bound, select_blocks against
the fp64 reference under the comparison rule of tests/block_select_ref.py (white noise) and bit for bit (planted rankings, exact
ties), usp_block_select alone at its limit of key blocks and past it, the equivalence block_select= == block_mask=select_blocks(...)
on one device bit for bit, and through the basic ring (degree 2 and 4), Ulysses 2 and the 2 x 2 hybrid on one-device virtual grids."""
import ctypes
import os

import pytest
import torch

import block_select_inputs as X
import block_select_ref as SR
from golden_util import TOL, assert_close, grad_tol

pytestmark = pytest.mark.gpu
POISON = float("nan")


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def strided(t, dev):
    """`t` (B, S, H, D) as a strided view into one NaN-poisoned device buffer: another head beside it, the head dim in the upper
    half of a row of 2 D, a batch stride with slack -- every stride a multiple of 8 elements, the view 16-byte aligned."""
    B, S, H, D = t.shape
    buf = torch.full((B, S + 3, H + 1, 2 * D), POISON, dtype=t.dtype, device=dev)
    view = buf[:, 1:S + 1, :H, D:]
    view.copy_(t)
    return view


def guarded(shape, dev, fill=0xFF):
    """A uint8 tensor of `shape` pre-filled with `fill` between two guard runs of 64 bytes: (view, check)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device=dev)
    view = buf[64:64 + n].view(shape)
    view.fill_(fill)

    def check():
        assert bool((buf[:64] == 0xA5).all()) and bool((buf[64 + n:] == 0xA5).all()), "a guard byte was written"
    return view, check


# ---- 1. usp_block_means ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("S", [64, 300, 1024, 8300])
def test_block_means_against_fp64(dev, S, D, dtype):
    from yunchang_amd import _C
    g = torch.Generator().manual_seed(S + D)
    B = 2 if S <= 1024 else 1
    for H in (4, 2, 8, 1):                       # the q and k sides of GQA 4 / 2 and 8 / 1
        x = (torch.randn(B, S, H, D, generator=g) * 1.5 + 0.25).to(dtype)
        xv = strided(x, dev)
        nb = SR.n_blocks(S)
        out, check = guarded((B * nb * H * D * 4,), dev)
        out32 = out.view(torch.float32).view(B, nb, H, D)
        _C.block_means(xv, out=out32)
        check()
        ref, tol = SR.mean_tolerance(x)
        err = (out32.cpu().double() - ref).abs()
        assert not torch.isnan(out32).any(), "a poisoned element was read"
        frac = float((err / (tol * (1 + 2.0 ** -10) + 1e-300)).max())
        print(f"MEANERR S={S} D={D} H={H} {dtype}: {frac:.3f} of the bound (largest |err| {float(err.max()):.3e})")
        assert frac <= 1.0
        # the order of every sum is a function of (row, d) alone: another grid (one batch entry, one head) gives the same bits
        assert torch.equal(_C.block_means(xv[B - 1:]), out32[B - 1:])
        assert torch.equal(_C.block_means(xv[:, :, H - 1:]), out32[:, :, H - 1:])
        assert torch.equal(_C.block_means(x.to(dev)), out32)             # ... and so does another layout


def test_block_means_head_dims_and_refusals(dev):
    from yunchang_amd import _C
    x = torch.randn(1, 200, 3, 96, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    got = _C.block_means(x.to(dev))                                       # any D % 8 == 0 up to 128
    ref, tol = SR.mean_tolerance(x)
    assert bool(((got.cpu().double() - ref).abs() <= tol * (1 + 2.0 ** -10)).all())
    with pytest.raises(RuntimeError, match="usp_block_means"):
        _C.block_means(torch.zeros(1, 128, 2, 40, dtype=torch.bfloat16, device=dev)[..., 1:33])   # off a 16-byte boundary


# ---- 2. select_blocks against the reference --------------------------------------------------------------------------------------------
def _run_grid(dev, q, k, planted):
    """Every (causal, top_k, keep_first, keep_local) of the grid through the two kernels, the mask in a 0xFF-filled guarded
    buffer; the public select_blocks on strided views for the first of them."""
    from yunchang_amd import _C
    from yunchang_amd.kernels.attention import select_blocks
    B, S, Hq, D = q.shape
    nb = SR.n_blocks(S)
    prob = SR.Problem(q, k)
    qd, kd = strided(q, dev), strided(k, dev)
    qbar, kbar = _C.block_means(qd), _C.block_means(kd)
    worst = 0.0
    for i, (causal, top_k, kf, kl) in enumerate(X.select_grid(nb)):
        out, check = guarded((B, Hq, nb, nb), dev)
        _C.block_select(qbar, kbar, top_k, D ** -0.5, causal, kf, kl, 0, out=out)
        check()
        assert bool((out <= 1).all()), "every byte is written, 0 or 1"
        got = out.bool().cpu()
        ref = prob.judge(top_k, causal, kf, kl)
        what = f"S={S} causal={causal} top_k={top_k} keep_first={kf} keep_local={kl}"
        if planted:
            assert torch.equal(got, ref.mask), what
        else:
            worst = max(worst, SR.compare(got, ref, what))
        if i % 7 == 0:
            pub = select_blocks(qd, kd, top_k, causal=causal, keep_first=kf, keep_local=kl)
            assert pub.dtype == torch.bool and not pub.requires_grad and torch.equal(pub.cpu(), got), what
    return prob, worst


@pytest.mark.parametrize("case", X.WHITE_CASES, ids=lambda c: f"S{c[0]}")
def test_select_blocks_white_noise(dev, case):
    from yunchang_amd import _C
    S, Hq, Hkv, D, dtype, seed = case
    q, k = X.white(1, S, Hq, Hkv, D, dtype, seed)
    prob, worst = _run_grid(dev, q, k, planted=False)
    # the measured score error against the derived bound: the kernel's scores from its own means, recomputed in fp64
    qbar, kbar = _C.block_means(q.to(dev)).cpu(), _C.block_means(k.to(dev)).cpu()
    s32 = SR.scores(qbar, kbar, D ** -0.5)
    err = (s32 - prob.s).abs()
    print(f"SELECT S={S} D={D}: ambiguous rows {worst:.4f}; |score(kernel means) - score64| max {float(err.max()):.3e}, "
          f"eps max {float(prob.eps.max()):.3e}, largest share of eps {float((err / prob.eps).max()):.3f}")
    assert bool((err <= prob.eps).all())


@pytest.mark.parametrize("case", X.PLANTED_CASES, ids=lambda c: f"S{c[0]}")
def test_select_blocks_planted(dev, case):
    S, Hq, Hkv, D, dtype, seed = case
    q, k, _, _ = X.planted(1, S, Hq, Hkv, D, dtype, seed)
    _run_grid(dev, q, k, planted=True)


def test_select_blocks_batch_and_ties(dev):
    from yunchang_amd.kernels.attention import select_blocks
    q, k, _, _ = X.planted(2, 1024, 8, 2, 32, torch.bfloat16, 11)
    q[1] = q[1].flip(0)                                                  # another problem in the second batch entry: the rows reversed
    for causal in (True, False):
        got = select_blocks(q.to(dev), k.to(dev), 3, causal=causal, keep_first=1)
        assert torch.equal(got.cpu(), SR.select_ref(q, k, 3, None, causal, 1, 1)), causal
    q0, k0 = X.zero_q(1, 1024, 4, 2, 32)
    qt, kt = X.twins(1, 1024, 4, 2, 32, 2, 5)
    for (q, k) in ((q0, k0), (qt, kt)):
        for causal, top_k, kf, kl in X.select_grid(8):
            got = select_blocks(q.to(dev), k.to(dev), top_k, causal=causal, keep_first=kf, keep_local=kl)
            assert torch.equal(got.cpu(), SR.select_ref(q, k, top_k, None, causal, kf, kl)), (causal, top_k, kf, kl)


# ---- 3. the C entry point alone, at its limit and past it -------------------------------------------------------------------------------
def _limit_problem(nbk, nbq, dev):
    """Means given directly: D = 32, one head; kbar[J] = value[J] e_0, qbar[I] = (1 + I) e_0, so score = scale (1 + I) value[J],
    exact in fp32 and strictly ordered: the winners 2 + m / 16 at J = 0, nbk - 1 and both sides of the selection loop's
    256-block passes, everything else a permutation of the grid j / 16384."""
    g = torch.Generator().manual_seed(nbk)
    value = torch.randperm(nbk, generator=g).double() / 16384.0
    winners = [255, 256, 511, 512, nbk - 257, nbk - 256, 0, nbk - 1]
    for m, J in enumerate(winners):
        value[J] = 2.0 + m / 16.0
    kbar = torch.zeros(1, nbk, 1, 32, dtype=torch.float32)
    kbar[0, :, 0, 0] = value.float()
    qbar = torch.zeros(1, nbq, 1, 32, dtype=torch.float32)
    qbar[0, :, 0, 0] = 1.0 + torch.arange(nbq, dtype=torch.float32)
    return qbar.to(dev), kbar.to(dev), winners


def test_c_entry_at_the_limit_of_key_blocks(dev):
    from yunchang_amd import _C
    nbk, nbq = _C.BLOCK_SELECT_MAX_BLOCKS, 4
    qbar, kbar, winners = _limit_problem(nbk, nbq, dev)
    for causal, top_k, kf, kl in ((False, 6, 0, 1), (False, 12, 0, 1), (True, 9, 1, 2), (False, 0, 0, 0), (False, nbk + 1, 0, 1)):
        out, check = guarded((1, 1, nbq, nbk), dev)
        _C.block_select(qbar, kbar, top_k, 0.25, causal, kf, kl, nbk - nbq, out=out)
        check()
        want = SR.select_from_scores(SR.scores(qbar.cpu(), kbar.cpu(), 0.25), top_k, causal, kf, kl, nbk - nbq)
        assert torch.equal(out.bool().cpu(), want), (causal, top_k, kf, kl)
        if top_k == 6 and not causal:                                    # 1 forced + the five best winners, the ends included
            assert want[0, 0, 0].nonzero()[:, 0].tolist() == [0, 512, nbk - 257, nbk - 256, nbk - nbq, nbk - 1]
    # every score equal: the cut falls inside one run of ties that spans several passes -- the lowest J win
    kbar[0, :, 0, 0] = 1.0
    out, check = guarded((1, 1, nbq, nbk), dev)
    _C.block_select(qbar, kbar, 700, 0.25, False, 0, 1, nbk - nbq, out=out)
    check()
    want = torch.zeros(nbq, nbk, dtype=torch.bool)
    want[:, :699] = True
    want[torch.arange(nbq), nbk - nbq + torch.arange(nbq)] = True
    assert torch.equal(out.bool().cpu()[0, 0], want)


def test_c_entry_past_the_limit_is_unsupported_and_writes_nothing(dev):
    from yunchang_amd import _C
    nbk = _C.BLOCK_SELECT_MAX_BLOCKS + 1
    qbar, kbar, _ = _limit_problem(nbk, 4, dev)
    out, check = guarded((1, 1, 4, nbk), dev)
    fn = _C._select_entry("usp_block_select")
    rc = fn(qbar.data_ptr(), kbar.data_ptr(), 1, 1, 1, 32, 4, nbk, nbk - 4, 0.25, 0, 3, 0, 1, out.data_ptr(), out.stride(0),
            out.stride(1), out.stride(2), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -2
    check()
    assert bool((out == 0xFF).all()), "the mask is untouched"
    with pytest.raises(RuntimeError, match="usp_block_select"):
        _C.block_select(qbar, kbar, 3, 0.25, False, 0, 1, nbk - 4)


# ---- 4. block_select= is block_mask=select_blocks(...) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("S,Hq,Hkv,D,causal", [(1024, 4, 2, 64, True), (300, 4, 2, 96, False)], ids=["S1024-causal", "S300-D96-full"])
def test_one_device_equivalence_bit_for_bit(dev, S, Hq, Hkv, D, causal):
    import yunchang_amd as Y
    from yunchang_amd import _C
    from yunchang_amd.kernels.attention import hip_attn_forward, hip_attn_func, select_blocks
    g = torch.Generator().manual_seed(S)
    q, k, v, do = (torch.randn(1, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv, Hq))
    sel = Y.BlockSelect(3, 1, 1)
    runs = {}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                               # nothing on the call path reads the device
    try:
        for name in ("select", "mask"):
            lq, lk, lv = (t.clone().requires_grad_(True) for t in (q, k, v))
            kw = dict(block_select=sel) if name == "select" else \
                dict(block_mask=select_blocks(lq, lk, 3, causal=causal, keep_first=1, keep_local=1))
            out, lse, _ = hip_attn_func(lq, lk, lv, causal=causal, return_attn_probs=True, **kw)
            kinds = _C.last_launch_kinds()
            out.backward(do)
            runs[name] = (out.detach(), lse, lq.grad, lk.grad, lv.grad, kinds)
            fo, fl = hip_attn_forward(q, k, v, causal=causal, **kw)
            runs[name + "_fwd"] = (fo, fl, _C.last_launch_kinds())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in (("select", "mask"), ("select_fwd", "mask_fwd")):
        assert runs[a][-1] == runs[b][-1] and runs[a][-1], (runs[a][-1], runs[b][-1])
        for x, y, what in zip(runs[a][:-1], runs[b][:-1], ("out", "lse", "dq", "dk", "dv")):
            assert torch.equal(x, y), f"{a} vs {b}: {what}"
    assert torch.equal(runs["select"][0], runs["select_fwd"][0])
    # ... and it is block-sparse attention under the reference's mask
    import block_mask_ref as BR
    mask = select_blocks(q, k, 3, causal=causal, keep_first=1, keep_local=1)
    ref = BR.ref_all(do, q, k, v, D ** -0.5, mask, causal)
    assert_close(runs["select"][0], ref[0], *TOL["bfloat16"]["out"], "out")
    for got, want, name in zip(runs["select"][2:5], ref[2:], ("dq", "dk", "dv")):
        assert_close(got, want, *grad_tol("bfloat16", Hq // Hkv), name)


def test_none_is_the_plain_call(dev):
    from yunchang_amd import _C
    from yunchang_amd.kernels.attention import hip_attn_forward, hip_attn_func
    g = torch.Generator().manual_seed(5)
    q, k, v, do = (torch.randn(1, 512, h, 64, generator=g).to(torch.bfloat16).to(dev) for h in (4, 2, 2, 4))
    res = []
    for kw in ({}, dict(block_select=None)):
        lq, lk, lv = (t.clone().requires_grad_(True) for t in (q, k, v))
        out = hip_attn_func(lq, lk, lv, causal=True, **kw)
        kinds = _C.last_launch_kinds()
        out.backward(do)
        res.append((out.detach(), lq.grad, lk.grad, lv.grad, hip_attn_forward(q, k, v, causal=True, **kw)[1], kinds))
    assert res[0][-1] == res[1][-1]
    for x, y in zip(res[0][:-1], res[1][:-1]):
        assert torch.equal(x, y)


# ---- 5. rings and layers on one-device virtual grids -------------------------------------------------------------------------------------
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


def gather_grid(ud, rd, real_dist):
    """tests/virtual_grid.py's grid with the one collective the selection adds: all_gather_into_tensor over a ring group, as one
    grouped self send / recv behind every member's stream."""
    from virtual_grid import Group, VirtualGrid

    class GatherGrid(VirtualGrid):
        def all_gather_into_tensor(self, out, inp, group=None):
            assert isinstance(group, Group) and group.kind == "ring"
            P = len(group.members)
            self.calls.append(("gather", self.tls.rank))

            def pairs_of(per_rank):                                 # member s's input -> chunk s of every member's output
                return [(per_rank[s][0], per_rank[d][1].chunk(P)[si]) for si, s in enumerate(group.members) for d in group.members]
            done = self._joint(group, (inp, out), pairs_of)
            if done is not None:
                torch.cuda.current_stream().wait_event(done)
    return GatherGrid(ud, rd, real_dist)


def ring_problem(dev, seed=17):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(1, 1024, h, 64, generator=g).to(torch.bfloat16).to(dev) for h in (4, 2, 2, 4))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("ud,rd,kind", [(1, 2, "ring"), (1, 4, "ring"), (2, 1, "ulysses"), (2, 2, "hybrid")],
                         ids=["ring2", "ring4", "ulysses2", "hybrid2x2"])
def test_rings_and_layers_on_virtual_grids(dev, nccl_single, monkeypatch, ud, rd, kind, causal):
    """Every virtual rank runs the public call under block_select= (the ring function; the layer's forward) and then the same
    steps by hand -- exchange, select_block_rows, ring forward and backward under the selected rows-only mask (autograd keeps one
    worker thread per device, on which virtual ranks cannot wait for each other).  The rank's mask is, bit for bit, its rows and
    heads of the single-device select_blocks; the public call's out is the hand-made one; out and gradients are the
    single-device block_mask= results within the tolerances of the block-mask ring tests."""
    import yunchang_amd as Y
    import yunchang_amd.hybrid.attn_layer as HL
    import yunchang_amd.ring.front_end as FE
    import yunchang_amd.ring.ring_flash_attn as RF
    import yunchang_amd.ulysses.attn_layer as UL
    from yunchang_amd.comm.all_to_all import SeqAllToAll4D, SeqAllToAll4DKV, local_heads
    from yunchang_amd.kernels.attention import hip_attn_backward, hip_attn_forward, select_blocks
    from virtual_grid import Ctx, patch_dist, run_grid
    q, k, v, do = ring_problem(dev)
    S, Hq, D = q.shape[1], q.shape[2], q.shape[3]
    ws, scale = ud * rd, D ** -0.5
    rows = S // ws
    sel = Y.BlockSelect(3, 1, 1)
    grid = gather_grid(ud, rd, nccl_single)
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
        elif kind == "hybrid":
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
        to_heads = lambda t, fn=SeqAllToAll4D: t if ud == 1 else fn.forward(Ctx(), upg, t, 2, 1, False, False)
        to_seq = lambda t: t if ud == 1 else SeqAllToAll4D.forward(Ctx(), upg, t, 1, 2, False, False)
        with torch.cuda.stream(streams[r]), torch.no_grad():
            if kind == "ring":
                out = RF.ring_flash_attn_func(lq, lk, lv, causal=causal, block_select=sel, group=rpg)
            else:
                out = layers[r](lq, lk, lv, causal=causal, block_select=sel)
            q2, k2, v2, do2 = to_heads(lq), to_heads(lk, SeqAllToAll4DKV), to_heads(lv, SeqAllToAll4DKV), to_heads(ldo)
            bm = FE.select_block_rows(q2, k2, sel, scale, causal, rpg)
            assert bm.rows_only == (rd > 1)
            o2, lse = RF.ring_flash_attn_forward(rpg, q2, k2, v2, scale, causal=causal, cu_doclens=bm)
            g2 = RF.ring_flash_attn_backward(rpg, do2, q2, k2, v2, o2, lse, scale, causal=causal, cu_doclens=bm)
            return [out, to_seq(o2)] + [to_seq(g.contiguous()) for g in g2[:3]] + [bm.mask]
    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    whole = select_blocks(q, k, 3, causal=causal, keep_first=1, keep_local=1)
    one = list(hip_attn_forward(q, k, v, causal=causal, block_mask=whole))
    g1 = [torch.empty_like(t) for t in (q, k, v)]
    hip_attn_backward(do, q, k, v, one[0], one[1], *g1, bwd_causal=causal, block_mask=whole)
    tol_o, tol_g = TOL["bfloat16"]["out"], grad_tol("bfloat16", 2)
    n = (S // rd) // 128
    if rd > 1:
        assert sum(1 for c in grid.calls if c[0] == "gather") == 2 * ws, "one all-gather of the pooled keys per call"
    for r in range(ws):
        u, rr = r % ud, r // ud
        sl = slice(r * rows, (r + 1) * rows)
        out, out_hand, dq, dk, dv, mask = res[r]
        assert torch.equal(mask, whole[:, local_heads(Hq, ud, u), rr * n:(rr + 1) * n, :]), f"rank {r}: its rows of the selection"
        assert torch.equal(out, out_hand), f"rank {r}: the public call and its steps by hand"
        assert_close(out, one[0][:, sl].double(), 2 * tol_o[0], 2 * tol_o[1], f"{kind} {ud}x{rd} rank {r} out vs one device")
        for got, single, name in ((dq, g1[0], "dq"), (dk, g1[1], "dk"), (dv, g1[2], "dv")):
            assert_close(got, single[:, sl].double(), 2 * tol_g[0], 2 * tol_g[1], f"{kind} {ud}x{rd} rank {r} {name} vs one device")


@pytest.mark.parametrize("layer", ["basic", "zigzag", "strip", "ulysses", "qkvpacked"])
def test_layers_at_degree_one_with_autograd(dev, nccl_single, layer):
    """The public layers on a 1-rank grid, forward and autograd backward: bit for bit the block_mask= call."""
    import yunchang_amd as Y
    from yunchang_amd.kernels.attention import select_blocks
    q, k, v, do = ring_problem(dev, seed=23)
    Y.set_seq_parallel_pg(1, 1, 0, 1)
    sel = Y.BlockSelect(3, 1, 1)
    res = []
    for use_select in (True, False):
        if layer == "qkvpacked":
            kk, vv = (t.repeat_interleave(2, dim=2) for t in (k, v))
            qkv = torch.stack([q, kk, vv], dim=2).requires_grad_(True)
            kw = dict(block_select=sel) if use_select else dict(block_mask=select_blocks(q, kk, 3, causal=True, keep_first=1))
            out = Y.LongContextAttentionQKVPacked(ring_impl_type="basic", attn_type=Y.AttnType.HIP)(qkv, causal=True, **kw)
            out.backward(do)
            res.append([out.detach(), qkv.grad])
        else:
            tq, tk, tv = (t.clone().requires_grad_(True) for t in (q, k, v))
            kw = dict(block_select=sel) if use_select else dict(block_mask=select_blocks(q, k, 3, causal=True, keep_first=1))
            if layer == "ulysses":
                import torch.distributed as dist
                attn = Y.UlyssesAttention(dist.group.WORLD, attn_type=Y.AttnType.HIP)
            else:
                attn = Y.LongContextAttention(ring_impl_type=layer, attn_type=Y.AttnType.HIP)
            out = attn(tq, tk, tv, causal=True, **kw)
            out.backward(do)
            res.append([out.detach(), tq.grad, tk.grad, tv.grad])
    for x, y in zip(*res):
        assert torch.equal(x, y), layer
