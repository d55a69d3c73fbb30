"""Block attention mass on the GPU: usp_block_attn_mass against the fp64 reference within the derived bound
(tests/block_mass_ref.py) on ragged, multi-block and GQA shapes through strided, poisoned, guarded layouts; launch depth; bit
identity of repeated calls and of a ring's slice launches; the keyword on the single-device calls; rings and layers on
one-device virtual grids; recall."""
import os

import numpy as np
import pytest
import torch

import block_mass_ref as MR
import layout_util as LU

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
GUARD = 0x7FA5A5A5          # a NaN: an element that was never written is seen


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def problem(B, S, Hq, Hkv, D, dtype, dev, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * S + D)
    return tuple(torch.randn(B, S, h, D, generator=g).to(DT[dtype]).to(dev) for h in (Hq, Hkv))


def forward_lse(q, k, causal):
    """The lse of the attention call itself, as the kernels write it."""
    from yunchang_amd.kernels.attention import hip_attn_forward
    return hip_attn_forward(q, k, k, causal=causal)[1]


def guarded_out(B, Hq, nbq, nbk, dev):
    """An fp32 (B, Hq, nbq, nbk) view with slack in every stride inside a NaN-filled buffer between guard words: (view, check);
    check(): the guard words and every element outside the view are intact, every element of the view was written."""
    shape = (B, Hq + 1, nbq + 2, nbk + 5)
    n = int(np.prod(shape))
    raw = torch.full((n + 128,), GUARD, dtype=torch.int32, device=dev)
    body = raw[64:64 + n].view(shape)
    view = body.view(torch.float32)[:, :Hq, 1:nbq + 1, :nbk]

    def check():
        assert bool((raw[:64] == GUARD).all()) and bool((raw[64 + n:] == GUARD).all()), "a guard word was written"
        outside = body.clone()
        outside[:, :Hq, 1:nbq + 1, :nbk] = GUARD
        assert bool((outside == GUARD).all()), "an element outside the view was written"
        assert not bool(torch.isnan(view).any()), "an element of the view was not written"
    return view, check


def run_strided(q, k, lse, scale, causal, dev, index, diag=0):
    """One call of the entry point with every tensor a strided view into poisoned memory (tests/layout_util.py) and `out`
    between guard words."""
    from yunchang_amd import _C
    rs = np.random.RandomState(1000 + index)
    B = q.shape[0]
    arena = LU.Arena(dev)
    qv = LU.place(q, LU.draw_layout(rs, "in16", B), arena, "q")
    kv = LU.place(k, LU.draw_layout(rs, "in16", B), arena, "k")
    lv = LU.place(lse, LU.draw_layout(rs, "lse", B), arena, "lse")
    nbq, nbk = (q.shape[1] + 127) // 128, (k.shape[1] + 127) // 128
    out, check = guarded_out(B, q.shape[2], nbq, nbk, dev)
    _C.block_attn_mass(qv, kv, lv, scale, causal, diag, out=out)
    torch.cuda.synchronize()
    check()
    assert arena.unchanged() and arena.untouched(), arena.violations()
    return out.clone()


# ---- 1. the kernel against the reference -------------------------------------------------------------------------------------
SIZES = [64, 128, 129, 257, 300, 320, 449, 1024]
FORMS = [(D, dt) for D in (32, 64, 128) for dt in ("bf16", "fp16")]
HEADS = [(4, 2), (2, 1), (2, 2)]
CASES = [(S, causal, FORMS[(i + 2 * c) % 6], HEADS[(i + c) % 3]) for i, S in enumerate(SIZES) for c, causal in enumerate((True, False))]
CASES += [(S, causal, form, heads) for form in FORMS for heads in HEADS for S, causal in ((449, True), (300, False))
          if (S, causal, form, heads) not in CASES]


@pytest.mark.parametrize("S,causal,form,heads", CASES,
                         ids=[f"S{S}-{'causal' if c else 'full'}-D{f[0]}-{f[1]}-H{h[0]}x{h[1]}" for S, c, f, h in CASES])
def test_kernel_against_reference(dev, S, causal, form, heads):
    D, dtype = form
    q, k = problem(2, S, heads[0], heads[1], D, dtype, dev)
    scale = D ** -0.5
    lse = forward_lse(q, k, causal)
    got = run_strided(q, k, lse, scale, causal, dev, CASES.index((S, causal, form, heads)))
    ref = MR.mass_ref(q, k, lse, scale, causal)
    MR.check(got, ref, MR.exponent_error(q, k, lse, scale), f"S{S} causal={causal} D{D} {dtype} H{heads}")
    if causal:
        assert float(got.triu(1).abs().max()) == 0.0, "blocks above the diagonal are written as 0"


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_rows_without_mass_and_a_foreign_lse(dev, causal):
    """lse rows of -inf contribute 0 (the rest of their block still divides by rows(I)); a shifted lse -- what a call with sinks
    hands over -- scales the map: the function takes whatever lse it is given."""
    q, k = problem(2, 449, 4, 2, 64, "bf16", dev, seed=3)
    scale = 64 ** -0.5
    lse = forward_lse(q, k, causal).clone()
    lse[:, :, 5] = float("-inf")
    lse[:, 1, 128:256] = float("-inf")          # a whole row block of one head
    lse[:, :, 384:] = float("-inf")             # every row of the ragged last block
    lse[:, 2] += 0.75
    got = run_strided(q, k, lse, scale, causal, dev, 77 + causal)
    ref = MR.mass_ref(q, k, lse, scale, causal)
    MR.check(got, ref, MR.exponent_error(q, k, lse, scale), f"-inf rows causal={causal}")
    assert float(got[:, 1, 1].abs().max()) == 0.0 and float(got[:, :, 3].abs().max()) == 0.0


def test_launch_depth(dev):
    """More items than the launched workgroups hold at once (B 1, Hq 16, S 8192: 1024 items on two workgroups per CU): the
    persistent walk reaches every item.  The reference is taken head by head on the device, in fp64."""
    from yunchang_amd import _C
    q, k = problem(1, 8192, 16, 4, 64, "bf16", dev, seed=5)
    scale = 64 ** -0.5
    lse = forward_lse(q, k, True)
    got = _C.block_attn_mass(q, k, lse, scale, True)
    worst = 0.0
    for h in range(16):
        qh, kh, lh = q[:, :, h:h + 1], k[:, :, h // 4:h // 4 + 1], lse[:, h:h + 1]
        ref = MR.mass_ref(qh, kh, lh, scale, True)
        worst = max(worst, MR.check(got[:, h:h + 1], ref, MR.exponent_error(qh, kh, lh, scale), f"depth head {h}"))
    assert torch.equal(got, _C.block_attn_mass(q, k, lse, scale, True))
    print(f"MASSERR launch depth: worst {worst:.3f} of the bound")


# ---- 2. bit identity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("Sl,P", [(256, 2), (512, 2), (256, 4), (512, 4)])
def test_slice_launches_are_the_sub_matrices(dev, Sl, P, causal):
    """A launch on the rows of ring rank r against the keys of ring rank c with diag = (r - c) * S_local gives bit for bit the
    sub-matrix of the whole call -- zeros above the diagonal included -- through a column slice of one result; repeated calls
    and other batch / head counts give the same bits."""
    from yunchang_amd import _C
    S = Sl * P
    q, k = problem(2, S, 4, 2, 64, "bf16", dev, seed=9)
    scale = 64 ** -0.5
    lse = forward_lse(q, k, causal)
    whole = _C.block_attn_mass(q, k, lse, scale, causal)
    assert torch.equal(whole, _C.block_attn_mass(q, k, lse, scale, causal)), "repeated calls"
    one = _C.block_attn_mass(q[1:, :, 2:3], k[1:, :, 1:2], lse[1:, 2:3].contiguous(), scale, causal)
    assert torch.equal(one, whole[1:, 2:3]), "the result does not depend on B, H or the grid"
    n = Sl // 128
    for r in range(P):
        rows = torch.full((2, 4, n, P * n), float("nan"), device=dev)
        for c in range(P):
            _C.block_attn_mass(q[:, r * Sl:(r + 1) * Sl], k[:, c * Sl:(c + 1) * Sl], lse[:, :, r * Sl:(r + 1) * Sl].contiguous(), scale,
                               causal, (r - c) * Sl, out=rows[..., c * n:(c + 1) * n])
        assert torch.equal(rows, whole[:, :, r * n:(r + 1) * n]), (r, "slices against the whole call")
        if causal and r + 1 < P:
            assert float(rows[..., (r + 1) * n:].abs().max()) == 0.0


# ---- 3. the keyword on the single-device calls --------------------------------------------------------------------------------
@pytest.mark.parametrize("D,causal", [(64, True), (128, False), (80, True)])
def test_keyword_on_single_device_calls(dev, D, causal):
    from yunchang_amd.kernels.attention import block_attention_mass, hip_attn_forward, hip_attn_func
    g = torch.Generator().manual_seed(31 + D)
    q, k, v, do = (torch.randn(2, 449, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (4, 2, 2, 4))
    res = []
    for kw in (dict(), dict(return_block_mass=True)):
        lq, lk, lv = (t.clone().requires_grad_(True) for t in (q, k, v))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            r = hip_attn_func(lq, lk, lv, causal=causal, return_attn_probs=True, **kw)
            r[0].backward(do)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        res.append((r, lq.grad, lk.grad, lv.grad))
    (plain, *g0), (with_mass, *g1) = res
    assert len(plain) == 3 and len(with_mass) == 4 and with_mass[2] is None
    assert torch.equal(plain[0], with_mass[0]) and torch.equal(plain[1], with_mass[1]), "out and lse keep their bits"
    for a, b in zip(g0, g1):
        assert torch.equal(a, b), "dq, dk, dv keep their bits"
    mass = with_mass[3]
    assert mass.shape == (2, 4, 4, 4) and mass.dtype == torch.float32 and not mass.requires_grad
    assert torch.equal(mass, block_attention_mass(q, k, with_mass[1], causal=causal)), "the bits of block_attention_mass on the returned lse"
    out2, mass2 = hip_attn_func(q, k, v, causal=causal, return_block_mass=True)
    assert torch.equal(out2, plain[0]) and torch.equal(mass2, mass)
    o3, l3, m3 = hip_attn_forward(q, k, v, causal=causal, return_block_mass=True)
    assert torch.equal(m3, block_attention_mass(q, k, l3, causal=causal))
    ref = MR.mass_ref(q, k, with_mass[1], D ** -0.5, causal)
    MR.check(mass, ref, MR.exponent_error(q, k, with_mass[1], D ** -0.5), f"keyword D{D}")


# ---- 4. rings and layers on one-device virtual grids ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nccl_single():
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29743")
    own = not dist.is_initialized()
    if own:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    yield dist
    if own:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("ud,rd,kind", [(1, 2, "ring"), (1, 4, "ring"), (2, 1, "ulysses"), (2, 2, "hybrid")],
                         ids=["ring2", "ring4", "ulysses2", "hybrid2x2"])
def test_rings_and_layers_on_virtual_grids(dev, nccl_single, monkeypatch, ud, rd, kind, causal):
    """Every virtual rank runs the public call under return_block_mass=True, and the ring function by hand on the ring's lse:
    the rank's share is, bit for bit, its heads and its ring shard's row blocks of the single-device block_attention_mass on the
    lse the ranks hold; `out` keeps the bits of the call without the keyword; the map is within the bound of the reference."""
    import yunchang_amd as Y
    import yunchang_amd.hybrid.attn_layer as HL
    import yunchang_amd.ring.front_end as FE
    import yunchang_amd.ring.ring_flash_attn as RF
    import yunchang_amd.ulysses.attn_layer as UL
    from yunchang_amd.comm.all_to_all import SeqAllToAll4D, SeqAllToAll4DKV, local_heads
    from yunchang_amd.kernels.attention import block_attention_mass
    from virtual_grid import Ctx, VirtualGrid, patch_dist, run_grid
    g = torch.Generator().manual_seed(17)
    q, k, v = (torch.randn(1, 1024, h, 64, generator=g).to(torch.bfloat16).to(dev) for h in (4, 2, 2))
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
        elif kind == "hybrid":
            lay = Y.LongContextAttention(ring_impl_type="basic", attn_type=Y.AttnType.HIP)
            lay.ulysses_pg, lay.ring_pg = upg, rpg
            layers.append(lay)
    loc = [[t[:, r * rows:(r + 1) * rows].contiguous() for t in (q, k, v)] for r in range(ws)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(ws)]
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        upg, rpg = grid.groups_of(r)
        lq, lk, lv = loc[r]
        to_heads = lambda t, fn=SeqAllToAll4D: t if ud == 1 else fn.forward(Ctx(), upg, t, 2, 1, False, False)
        with torch.cuda.stream(streams[r]), torch.no_grad():
            if kind == "ring":
                plain = RF.ring_flash_attn_func(lq, lk, lv, causal=causal, group=rpg)
                out, mass = RF.ring_flash_attn_func(lq, lk, lv, causal=causal, return_block_mass=True, group=rpg)
            else:
                plain = layers[r](lq, lk, lv, causal=causal)
                out, mass = layers[r](lq, lk, lv, causal=causal, return_block_mass=True)
            q2, k2, v2 = to_heads(lq), to_heads(lk, SeqAllToAll4DKV), to_heads(lv, SeqAllToAll4DKV)
            _, lse = RF.ring_flash_attn_forward(rpg, q2, k2, v2, scale, causal=causal)
            hand = FE.ring_block_attention_mass(q2, k2, lse, softmax_scale=scale, causal=causal, group=rpg)
            return [plain, out, mass, hand, lse]
    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    Sl = S // rd
    n, nb = Sl // 128, S // 128
    lse_all = torch.empty(1, Hq, S, dtype=torch.float32, device=dev)
    for r in range(ws):
        u, rr = r % ud, r // ud
        lse_all[:, local_heads(Hq, ud, u), rr * Sl:(rr + 1) * Sl] = res[r][4]
    whole = block_attention_mass(q, k, lse_all, causal=causal)
    MR.check(whole, MR.mass_ref(q, k, lse_all, scale, causal), MR.exponent_error(q, k, lse_all, scale), f"{kind} {ud}x{rd}")
    for r in range(ws):
        u, rr = r % ud, r // ud
        plain, out, mass, hand, _ = res[r]
        want = whole[:, local_heads(Hq, ud, u), rr * n:(rr + 1) * n, :]
        assert mass.shape == (1, Hq // ud, n, nb) and mass.dtype == torch.float32
        assert torch.equal(out, plain), f"rank {r}: out keeps its bits"
        assert torch.equal(mass, hand), f"rank {r}: the public call and the ring function by hand"
        assert torch.equal(mass, want), f"rank {r}: its share of the single-device map"


@pytest.mark.parametrize("layer", ["basic", "zigzag", "strip", "ulysses", "qkvpacked"])
def test_layers_at_degree_one(dev, nccl_single, layer):
    """The public layers on a 1-rank grid, with autograd: (out, mass), mass the bits of block_attention_mass on the call's lse."""
    import yunchang_amd as Y
    from yunchang_amd.kernels.attention import block_attention_mass, hip_attn_func
    g = torch.Generator().manual_seed(23)
    q, k, v, do = (torch.randn(1, 450, h, 64, generator=g).to(torch.bfloat16).to(dev) for h in (4, 2, 2, 4))   # (zigzag: an even length)
    Y.set_seq_parallel_pg(1, 1, 0, 1)
    if layer == "qkvpacked":
        k, v = (t.repeat_interleave(2, dim=2) for t in (k, v))
        qkv = torch.stack([q, k, v], dim=2).requires_grad_(True)
        out, mass = Y.LongContextAttentionQKVPacked(ring_impl_type="basic", attn_type=Y.AttnType.HIP)(qkv, causal=True, return_block_mass=True)
    else:
        lq = q.clone().requires_grad_(True)
        lay = Y.UlyssesAttention(None, attn_type=Y.AttnType.HIP) if layer == "ulysses" else \
            Y.LongContextAttention(ring_impl_type=layer, attn_type=Y.AttnType.HIP)
        out, mass = lay(lq, k, v, causal=True, return_block_mass=True)
    out.backward(do)
    ref_out, lse, _ = hip_attn_func(q, k, v, causal=True, return_attn_probs=True)
    assert not mass.requires_grad and mass.shape == (1, 4, 4, 4)
    assert torch.equal(mass, block_attention_mass(q, k, lse, causal=True))
    assert torch.equal(out, ref_out), "out is the call's without the keyword"


# ---- 5. recall ----------------------------------------------------------------------------------------------------------------
def planted_tokens(nbk, dev, noise=1.0):
    """Token-level q (1, 128 nbk, 2, 32) and k (1, 128 nbk, 1, 32) whose block means are the planted means of
    tests/block_select_top_p_inputs.py (times sqrt(PLANTED_SCALE), so the pooled scores lie where that file puts them at its
    peaked scale) under unit white noise."""
    import block_select_top_p_inputs as TX
    qbar, kbar = TX.synthetic_means(nbk)
    g = torch.Generator().manual_seed(900 + nbk)
    amp = TX.PLANTED_SCALE ** 0.5
    nbq = qbar.shape[1]
    rows = lambda m, n: (amp * m).repeat_interleave(128, dim=1)[:, :128 * n]
    qb = torch.cat([qbar, qbar[:, -1:].expand(-1, nbk - nbq, -1, -1)], dim=1) if nbq < nbk else qbar
    q = rows(qb, nbk) + noise * torch.randn(1, 128 * nbk, 2, 32, generator=g)
    k = rows(kbar, nbk) + noise * torch.randn(1, 128 * nbk, 1, 32, generator=g)
    return q.to(torch.bfloat16).to(dev), k.to(torch.bfloat16).to(dev)


def test_recall(dev):
    """block_mask_recall of an all-set mask is the row sum: 1 within the bound.  The recall of the top-p gate on a planted input
    is reported, not asserted."""
    import yunchang_amd as Y
    from yunchang_amd.kernels.attention import block_attention_mass, block_mask_recall, hip_attn_func, select_blocks_top_p
    q, k = problem(1, 1024, 4, 2, 64, "bf16", dev, seed=41)
    scale = 64 ** -0.5
    _, lse, _ = hip_attn_func(q, k, k, causal=True, return_attn_probs=True)
    mass = block_attention_mass(q, k, lse, causal=True)
    ones = torch.ones(8, 8, dtype=torch.bool, device=dev)
    full = block_mask_recall(mass, ones)
    assert full.shape == (1, 4, 8) and torch.equal(full, mass.sum(-1))
    ref = MR.mass_ref(q, k, lse, scale, True)
    tol = MR.tolerance(ref, MR.exponent_error(q, k, lse, scale)).sum(-1) + 8 * 2.0 ** -24
    # the reference's own rows sum to 1 up to the fp32 rounding of the lse it was handed: |lse| 2^-24 relative
    lse_term = lse.abs().amax().item() * 2.0 ** -23
    assert bool(((full.double() - 1).abs() <= tol + lse_term).all()), float((full.double() - 1).abs().max())
    top_p = 0.9
    for name, (pq, pk) in (("white noise S1024", (q, k)), ("planted nbk 5", planted_tokens(5, dev))):
        _, pl, _ = hip_attn_func(pq, pk, pk, causal=True, return_attn_probs=True)
        pm = block_attention_mass(pq, pk, pl, causal=True)
        mask = select_blocks_top_p(pq, pk, top_p, causal=True)
        rec = block_mask_recall(pm, mask)
        assert rec.shape == pm.shape[:3] and bool((rec <= pm.sum(-1) + 1e-6).all())
        nb = pm.shape[-1]
        kept = float(mask.float().tril().sum()) / (pm.shape[1] * nb * (nb + 1) / 2)
        print(f"RECALL {name} BlockSelectTopP({top_p}): kept {kept:.3f} of the blocks, recall min {float(rec.min()):.3f} "
              f"median {float(rec.median()):.3f} max {float(rec.max()):.3f}")
    assert Y.block_mask_recall is block_mask_recall
