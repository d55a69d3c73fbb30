"""Top-p block selection (`block_select=BlockSelectTopP(...)`) on the GPU: usp_block_select_top_p alone on synthetic means at the
chunk edges of its 256-thread passes, at two scales, at its limit of key blocks and past it; select_blocks_top_p end to end
against the fp64 reference under the acceptance rule of tests/block_select_top_p_ref.py (white noise) and bit for bit (planted
rankings, equal weights, twins, one block with all the mass); share_group; the equivalence block_select= ==
block_mask=select_blocks_top_p(...) on one device bit for bit, without a host read; and the basic ring (degree 2 and 4), Ulysses 2
and the 2 x 2 hybrid on one-device virtual grids."""
import ctypes

import pytest
import torch

import block_select_inputs as X
import block_select_ref as SR
import block_select_top_p_inputs as TX
import block_select_top_p_ref as TR
from golden_util import TOL, assert_close, grad_tol
from test_gpu_block_select import gather_grid, guarded, nccl_single, ring_problem, strided  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def strided_mask(B, Hq, nbq, nbk, dev):
    """A (B, Hq, nbq, nbk) uint8 view with slack in every stride inside a 0xFF-filled buffer between guard bytes."""
    buf, check = guarded((B, Hq + 1, nbq + 2, nbk + 5), dev)
    return buf[:, :Hq, 1:nbq + 1, :nbk], buf, check


def run_entry(qbar, kbar, scale, causal, row0, kf, kl, p, share, dev):
    """One call of the entry point into a strided, poisoned, guarded mask: the bool mask on the CPU."""
    from yunchang_amd import _C
    B, nbq, Hq, _ = qbar.shape
    nbk = kbar.shape[1]
    view, buf, check = strided_mask(B, Hq, nbq, nbk, dev)
    _C.block_select_top_p(qbar, kbar, p, scale, causal, kf, kl, share, row0, out=view)
    check()
    assert bool((view <= 1).all()), "every byte of the view is written, 0 or 1"
    outside = buf.clone()
    outside[:, :Hq, 1:nbq + 1, :nbk] = 0xFF
    assert bool((outside == 0xFF).all()), "a byte outside the view was written"
    return view.bool().cpu()


# ---- 1. the C entry point on synthetic means ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbk", TX.SYNTH_NBK)
def test_c_entry_on_synthetic_means(dev, nbk):
    qbar, kbar = TX.synthetic_means(nbk)
    qd, kd = qbar.to(dev), kbar.to(dev)
    for scale in (TX.SYNTH_D ** -0.5, TX.peaked_scale(qbar, kbar)):
        prob = TR.Problem(scale=scale, means=(qbar, kbar))
        judged, counts = [], []
        for causal, row0, kf, kl, p, share in TX.synth_grid(nbk):
            got = run_entry(qd, kd, scale, causal, row0, kf, kl, p, share, dev)
            j = prob.judge(p, causal, kf, kl, share, row0)
            TR.compare(got, j, f"nbk={nbk} scale={scale:.3f} causal={causal} row0={row0} kf={kf} kl={kl} p={p} share={share}")
            judged.append(j)
            counts.append(int(got.sum()))
        share_amb = TX.case_ambiguity(judged)
        print(f"TOPP synthetic nbk={nbk} scale={scale:.3f}: ambiguous rows {share_amb:.5f}, selected {min(counts)}..{max(counts)} per call")
        assert share_amb <= TX.CAP


def _limit_means(nbk, nbq, dev):
    """tests/test_gpu_block_select.py's limit problem: one head, D = 32, score = scale (1 + I) value[J], exact in fp32; eight
    winners 2 + m / 16 at J = 255, 256, 511, 512, nbk - 257, nbk - 256, 0, nbk - 1 over a permutation of the grid j / 16384."""
    from test_gpu_block_select import _limit_problem
    return _limit_problem(nbk, nbq, dev)


def test_c_entry_at_the_limit_of_key_blocks(dev):
    from yunchang_amd import _C
    nbk, nbq = _C.BLOCK_SELECT_MAX_BLOCKS, 4
    qbar, kbar, winners = _limit_means(nbk, nbq, dev)
    prob = TR.Problem(scale=4.0, means=(qbar.cpu(), kbar.cpu()))       # from row 1 on the winners carry nearly all the mass
    for causal, p, kf, kl, share in ((False, 0.9, 0, 1, False), (True, 0.5, 1, 2, True), (False, 0.05, 0, 0, False), (False, 1.0, 0, 1, False)):
        got = run_entry(qbar, kbar, 4.0, causal, nbk - nbq, kf, kl, p, share, dev)
        j = prob.judge(p, causal, kf, kl, share, nbk - nbq)
        TR.compare(got, j, f"limit causal={causal} p={p}")
        clear = ~j.ambiguous()                                           # (by the reference alone)
        assert (p == 1.0 or int(clear.sum()) >= 3) and torch.equal(got[clear], j.mask[clear]), (causal, p)
    # every weight equal (1 / 8192, exact): the cut falls inside one run of ties over all 32 passes -- the lowest J win, as many
    # as the tie expression asks for
    kbar[0, :, 0, 0] = 1.0
    got = run_entry(qbar, kbar, 0.25, False, nbk - nbq, 0, 1, 0.25, False, dev)
    for I in range(nbq):
        forced = torch.zeros(nbk, dtype=torch.bool)
        forced[nbk - nbq + I] = True
        need = TR.equal_weight_count(nbk, forced, 0.25)
        assert need == 2047, need
        want = forced.clone()
        want[:need] = True
        assert torch.equal(got[0, 0, I], want), I


def test_c_entry_past_the_limit_is_unsupported_and_writes_nothing(dev):
    from yunchang_amd import _C
    nbk = _C.BLOCK_SELECT_MAX_BLOCKS + 1
    qbar, kbar, _ = _limit_means(nbk, 4, dev)
    out, check = guarded((1, 1, 4, nbk), dev)
    fn = _C._select_top_p_entry("usp_block_select_top_p")
    rc = fn(qbar.data_ptr(), kbar.data_ptr(), 1, 1, 1, 32, 4, nbk, nbk - 4, 0.25, 0, 0.9, 0, 1, 0, out.data_ptr(), out.stride(0),
            out.stride(1), out.stride(2), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -2
    check()
    assert bool((out == 0xFF).all()), "the mask is untouched"
    with pytest.raises(RuntimeError, match="usp_block_select_top_p"):
        _C.block_select_top_p(qbar, kbar, 0.9, 0.25, False, 0, 1, False, nbk - 4)


# ---- 2. select_blocks_top_p end to end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.WHITE_CASES, ids=lambda c: f"S{c[0]}")
def test_select_blocks_top_p_white_noise(dev, case):
    from yunchang_amd.kernels.attention import select_blocks_top_p
    S, Hq, Hkv, D, dtype, seed = case
    q, k = X.white(1, S, Hq, Hkv, D, dtype, seed)
    prob = TR.Problem(q, k)
    qd, kd = strided(q, dev), strided(k, dev)
    judged = []
    for causal, kf, kl, p, share in TX.white_grid():
        got = select_blocks_top_p(qd, kd, p, causal=causal, keep_first=kf, keep_local=kl, share_group=share)
        assert got.dtype == torch.bool and not got.requires_grad and tuple(got.shape) == (1, Hq, SR.n_blocks(S), SR.n_blocks(S))
        j = prob.judge(p, causal, kf, kl, share)
        TR.compare(got.cpu(), j, f"S={S} causal={causal} kf={kf} kl={kl} p={p} share={share}")
        judged.append(j)
    share_amb = TX.case_ambiguity(judged)
    print(f"TOPP white S={S} D={D}: ambiguous rows {share_amb:.5f}")
    assert share_amb <= TX.CAP


@pytest.mark.parametrize("case", X.PLANTED_CASES, ids=lambda c: f"S{c[0]}")
def test_select_blocks_top_p_planted(dev, case):
    """Planted rankings at the default scale and at two where neighbouring weights differ by e^(1/4) and e: where the reference
    alone shows a selection unambiguous (every one but a handful), bit for bit."""
    from yunchang_amd.kernels.attention import select_blocks_top_p
    S, Hq, Hkv, D, dtype, seed = case
    q, k, _, _ = X.planted(1, S, Hq, Hkv, D, dtype, seed)
    qd, kd = q.to(dev), k.to(dev)
    exact = total = 0
    for scale in (None, TX.PLANTED_SCALE, 4 * TX.PLANTED_SCALE):
        prob = TR.Problem(q, k, scale)
        for causal, kf, kl, p, share in TX.white_grid():
            got = select_blocks_top_p(qd, kd, p, softmax_scale=scale, causal=causal, keep_first=kf, keep_local=kl, share_group=share).cpu()
            j = prob.judge(p, causal, kf, kl, share)
            TR.compare(got, j, f"planted S={S} scale={scale} causal={causal} kf={kf} kl={kl} p={p} share={share}")
            clear = ~j.ambiguous()
            assert torch.equal(got[clear], j.mask[clear]), (scale, causal, kf, kl, p, share)
            exact, total = exact + int(clear.sum()), total + clear.numel()
    print(f"TOPP planted S={S}: {exact} of {total} rows unambiguous by the reference alone, bit for bit")
    assert exact > total / 2


def test_exact_cases(dev):
    from yunchang_amd.kernels.attention import select_blocks_top_p
    # equal weights (q = 0): the forced blocks and the lowest-J others, as many as the tie expression gives
    q, k = X.zero_q(1, 1024, 4, 2, 32)
    for causal, kf, kl, p, share in TX.white_grid():
        got = select_blocks_top_p(q.to(dev), k.to(dev), p, causal=causal, keep_first=kf, keep_local=kl, share_group=share).cpu()
        visible, forced = SR.candidates(8, 8, causal, kf, kl)
        for I in range(8):
            nv = int(visible[I].sum())
            need = TR.equal_weight_count(nv, forced[I], p)
            # (share_group adds two heads' equal weights: every term doubles exactly, the count stays)
            cand = visible[I] & ~forced[I]
            want = forced[I] | (cand & (cand.cumsum(0) <= need))
            assert torch.equal(got[0, :, I], want.expand(4, 8)), (causal, kf, kl, p, share, I)
    # twins: key block 5 is a copy of key block 2 -- never selected without it
    q, k = X.twins(1, 1024, 4, 2, 32, 2, 5)
    for scale in (None, TX.PLANTED_SCALE):
        prob = TR.Problem(q, k, scale)
        for causal, kf, kl, p, share in TX.white_grid():
            got = select_blocks_top_p(q.to(dev), k.to(dev), p, softmax_scale=scale, causal=causal, keep_first=kf, keep_local=kl,
                                      share_group=share).cpu()
            j = prob.judge(p, causal, kf, kl, share)
            TR.compare(got, j, f"twins {scale} {causal} {kf} {kl} {p} {share}")
            both = j.cand[..., 2] & j.cand[..., 5]
            assert not bool((got[..., 5] & ~got[..., 2] & both).any())
    # a batch with another problem per entry
    q, k, _, _ = X.planted(2, 1024, 8, 2, 32, torch.bfloat16, 11)
    q[1] = q[1].flip(0)
    for causal in (True, False):
        got = select_blocks_top_p(q.to(dev), k.to(dev), 0.5, softmax_scale=TX.PLANTED_SCALE, causal=causal, keep_first=1).cpu()
        ref = TR.select_ref(q, k, 0.5, TX.PLANTED_SCALE, causal, 1, 1)
        assert torch.equal(got, ref) and not torch.equal(ref[0], ref[1]), causal


def test_one_block_carries_all_the_mass(dev):
    """kbar[J0] = e_0, every other key block -e_0, qbar = e_0, scale 200: the others' weights underflow to zero in fp32 (and are
    e^-400 in fp64).  Whatever top_p, 1.0 included: the forced blocks and J0."""
    nbk, nbq, J0 = 300, 3, 277
    kbar = torch.zeros(1, nbk, 1, 32)
    kbar[0, :, 0, 0] = -1.0
    kbar[0, J0, 0, 0] = 1.0
    qbar = torch.zeros(1, nbq, 2, 32)
    qbar[..., 0] = 1.0
    for p in TX.TOP_PS:
        for share in (False, True):
            for kf, kl in ((0, 1), (2, 2)):
                got = run_entry(qbar.to(dev), kbar.to(dev), 200.0, False, 10, kf, kl, p, share, dev)
                _, forced = SR.candidates(nbq, nbk, False, kf, kl, 10)
                want = forced.clone()
                want[:, J0] = True
                assert torch.equal(got, want.expand(1, 2, nbq, nbk)), (p, share, kf, kl)


# ---- 3. share_group -------------------------------------------------------------------------------------------------------------------------
def test_share_group(dev):
    from yunchang_amd.kernels.attention import select_blocks_top_p
    # G = 1: bit for bit the unshared selection
    q, k = X.white(2, 2100, 4, 4, 64, torch.bfloat16, 21)
    for causal in (True, False):
        for p in (0.3, 0.9):
            a = select_blocks_top_p(q.to(dev), k.to(dev), p, causal=causal, keep_first=1, share_group=True)
            b = select_blocks_top_p(q.to(dev), k.to(dev), p, causal=causal, keep_first=1, share_group=False)
            assert torch.equal(a, b), (causal, p)
    # Hq 8 / Hkv 2 and MQA against the reference at a scale that spreads the weights; all heads of a group identical (compare)
    for Hq, Hkv in ((8, 2), (8, 1)):
        q, k = X.white(1, 2100, Hq, Hkv, 64, torch.bfloat16, 22 + Hkv)
        prob = TR.Problem(q, k, 8.0)
        for causal in (True, False):
            for p in (0.3, 0.9):
                got = select_blocks_top_p(q.to(dev), k.to(dev), p, softmax_scale=8.0, causal=causal, share_group=True).cpu()
                j = prob.judge(p, causal, 0, 1, True)
                TR.compare(got, j, f"share {Hq}/{Hkv} causal={causal} p={p}")
                G = Hq // Hkv
                assert bool((got.view(1, Hkv, G, 17, 17) == got.view(1, Hkv, G, 17, 17)[:, :, :1]).all())
                unshared = select_blocks_top_p(q.to(dev), k.to(dev), p, softmax_scale=8.0, causal=causal).cpu()
                assert not torch.equal(unshared, got), "the heads of a group select differently on their own"


# ---- 4. block_select=BlockSelectTopP(...) is block_mask=select_blocks_top_p(...) -----------------------------------------------------------
@pytest.mark.parametrize("S,Hq,Hkv,D,causal", [(1024, 4, 2, 64, True), (300, 4, 2, 96, False)], ids=["S1024-causal", "S300-D96-full"])
def test_one_device_equivalence_bit_for_bit(dev, S, Hq, Hkv, D, causal):
    import yunchang_amd as Y
    from yunchang_amd import _C
    from yunchang_amd.kernels.attention import hip_attn_forward, hip_attn_func, select_blocks_top_p
    g = torch.Generator().manual_seed(S)
    q, k, v, do = (torch.randn(1, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv, Hq))
    sel = Y.BlockSelectTopP(0.6, 1, 1, True)
    runs = {}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                               # nothing on the call path reads the device
    try:
        for name in ("select", "mask"):
            lq, lk, lv = (t.clone().requires_grad_(True) for t in (q, k, v))
            kw = dict(block_select=sel) if name == "select" else \
                dict(block_mask=select_blocks_top_p(lq, lk, 0.6, causal=causal, keep_first=1, keep_local=1, share_group=True))
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
    # ... and it is block-sparse attention under a mask that keeps some blocks and drops some
    import block_mask_ref as BR
    mask = select_blocks_top_p(q, k, 0.6, causal=causal, keep_first=1, keep_local=1, share_group=True)
    nb = SR.n_blocks(S)
    kept = float(mask.float().sum()) / (Hq * (nb * (nb + 1) / 2 if causal else nb * nb))
    assert 0.3 < kept < 1.0, kept
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


# ---- 5. rings and layers on one-device virtual grids -----------------------------------------------------------------------------------------
def top_p_problem(dev, seed=17):
    return ring_problem(dev, seed)         # (unit white noise: nearly uniform weights, top_p 0.6 drops about 40 % of the blocks)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("causal,share", [(True, False), (False, True)], ids=["causal", "full-shared"])
@pytest.mark.parametrize("ud,rd,kind", [(1, 2, "ring"), (1, 4, "ring"), (2, 1, "ulysses"), (2, 2, "hybrid")],
                         ids=["ring2", "ring4", "ulysses2", "hybrid2x2"])
def test_rings_and_layers_on_virtual_grids(dev, nccl_single, monkeypatch, ud, rd, kind, causal, share):
    """tests/test_gpu_block_select.py::test_rings_and_layers_on_virtual_grids for the top-p record: every virtual rank runs the
    public call under block_select=BlockSelectTopP(...) and then the same steps by hand; the rank's rows-only mask is, bit for
    bit, its rows and heads of the single-device select_blocks_top_p; out and gradients are the single-device block_mask=
    results.  (4 query heads over 2 KV heads on 2 Ulysses ranks: whole groups per rank, so share_group is served.)"""
    import yunchang_amd as Y
    import yunchang_amd.hybrid.attn_layer as HL
    import yunchang_amd.ring.front_end as FE
    import yunchang_amd.ring.ring_flash_attn as RF
    import yunchang_amd.ulysses.attn_layer as UL
    from yunchang_amd.comm.all_to_all import SeqAllToAll4D, SeqAllToAll4DKV, local_heads
    from yunchang_amd.kernels.attention import hip_attn_backward, hip_attn_forward, select_blocks_top_p
    from virtual_grid import Ctx, patch_dist, run_grid
    q, k, v, do = top_p_problem(dev)
    S, Hq, D = q.shape[1], q.shape[2], q.shape[3]
    ws, scale = ud * rd, D ** -0.5
    rows = S // ws
    sel = Y.BlockSelectTopP(0.6, 1, 1, share)
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
    whole = select_blocks_top_p(q, k, 0.6, causal=causal, keep_first=1, keep_local=1, share_group=share)
    assert 0.2 < float(whole.float().mean()) < 0.9
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
    from yunchang_amd.kernels.attention import select_blocks_top_p
    q, k, v, do = top_p_problem(dev, seed=23)
    Y.set_seq_parallel_pg(1, 1, 0, 1)
    sel = Y.BlockSelectTopP(0.6, 1, 1, True)
    res = []
    for use_select in (True, False):
        if layer == "qkvpacked":
            kk, vv = (t.repeat_interleave(2, dim=2) for t in (k, v))
            qkv = torch.stack([q, kk, vv], dim=2).requires_grad_(True)
            kw = dict(block_select=sel) if use_select else \
                dict(block_mask=select_blocks_top_p(q, kk, 0.6, causal=True, keep_first=1, share_group=True))
            out = Y.LongContextAttentionQKVPacked(ring_impl_type="basic", attn_type=Y.AttnType.HIP)(qkv, causal=True, **kw)
            out.backward(do)
            res.append([out.detach(), qkv.grad])
        else:
            tq, tk, tv = (t.clone().requires_grad_(True) for t in (q, k, v))
            kw = dict(block_select=sel) if use_select else \
                dict(block_mask=select_blocks_top_p(q, k, 0.6, causal=True, keep_first=1, share_group=True))
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
