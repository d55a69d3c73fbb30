"""Head dims (192, 128) -- q and k of 192, v of 128: multi-head latent attention -- on the GPU (run with -m gpu on an MI355X): the
kernel family of csrc/usp_flash_fwd_qk192.hip and csrc/usp_flash_bwd_qk192.hip through hip_attn_forward / hip_attn_backward /
hip_attn_func and the C ABI binding, against plain fp64 attention (torch, autograd for the gradients) within the project's stated
tolerances (golden_util.TOL; lse 2e-3 / 1e-4; golden_util.long_sum_atol on gradient sums of >= 1000 products)."""
import numpy as np
import pytest
import torch

from golden_util import TOL, assert_close, long_sum_atol, round_to

pytestmark = pytest.mark.gpu
KINDS = {"fwd": ("fwd_qk192",), "bwd": ("dkdv_qk192", "dq_qk192")}
DQK, DV = 192, 128


@pytest.fixture(scope="module")
def dev():
    from yunchang_amd import _C
    _C.load()
    return torch.device("cuda:0")


def _inputs(B, Sq, Sk, Hq, Hkv, dt, dev, seed=0):
    """q, k, v, dout as 16-bit device tensors (values exactly representable, so the fp64 reference reads the same numbers)"""
    rs = np.random.RandomState(seed)
    shapes = [(B, Sq, Hq, DQK), (B, Sk, Hkv, DQK), (B, Sk, Hkv, DV), (B, Sq, Hq, DV)]
    return [torch.from_numpy(round_to(rs.standard_normal(s).astype(np.float32), dt)).to(getattr(torch, dt)).to(dev) for s in shapes]


def _ref(q, k, v, do, causal, scale=None):
    """fp64 attention with the bottom-right causal alignment: out, lse (-inf for a row that sees no key), dq, dk, dv"""
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    Sq, Sk, g = q.shape[1], k.shape[1], q.shape[2] // k.shape[2]
    s = torch.einsum("bthd,bshd->bhts", q, k.repeat_interleave(g, dim=2)) * (q.shape[-1] ** -0.5 if scale is None else scale)
    if causal:
        i, j = torch.arange(Sq, device=q.device)[:, None], torch.arange(Sk, device=q.device)[None, :]
        s = s.masked_fill(j > i + (Sk - Sq), float("-inf"))
    m = s.detach().amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    out = torch.einsum("bhts,bshd->bthd", e / l.clamp_min(1e-300), v.repeat_interleave(g, dim=2))
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), do.double())
    return dict(out=out.detach(), lse=(m + torch.log(l)).detach()[..., 0], dq=dq, dk=dk, dv=dv)


def _check(got, want, dt, Sq, Sk, G, what=""):
    for n, t in got.items():
        w = want[n]
        if n == "lse":
            fin = torch.isfinite(w)
            assert torch.equal(torch.isfinite(t), fin) and bool((t[~fin] == float("-inf")).all()), "empty rows must give lse = -inf"
            assert_close(t[fin].double(), w[fin], 2e-3, 1e-4, what + "lse")
            continue
        atol, rtol = TOL[dt]["out" if n == "out" else "grad"]
        if n != "out":
            atol = long_sum_atol(atol, Sk if n == "dq" else Sq * G, w)
        assert_close(t.double(), w, atol, rtol, what + n)


SHAPES = [
    # B, Sq, Sk, Hq, Hkv, causal, dtype
    (1, 1, 1, 1, 1, True, "float16"),
    (2, 77, 77, 2, 2, True, "bfloat16"),          # less than one item
    (1, 200, 333, 3, 1, True, "bfloat16"),        # ragged, bottom-right, GQA 3
    (1, 333, 200, 2, 2, True, "float16"),         # rows with no visible key
    (1, 384, 640, 4, 2, False, "bfloat16"),
    (1, 130, 1, 2, 1, False, "float16"),          # Sk = 1
    (1, 257, 193, 2, 1, True, "bfloat16"),        # one-row second forward item and third dQ item, one-key fourth tile
]


@pytest.mark.parametrize("B,Sq,Sk,Hq,Hkv,causal,dt", SHAPES)
def test_forward_backward_vs_fp64(dev, B, Sq, Sk, Hq, Hkv, causal, dt):
    from yunchang_amd import _C
    from yunchang_amd.kernels import hip_attn_backward, hip_attn_forward
    q, k, v, do = _inputs(B, Sq, Sk, Hq, Hkv, dt, dev)
    want = _ref(q, k, v, do, causal)
    out, lse = hip_attn_forward(q, k, v, 0.0, None, causal=causal)
    assert _C.last_launch_kinds() == KINDS["fwd"] and out.shape == (B, Sq, Hq, DV)
    empty = ~torch.isfinite(want["lse"]).transpose(1, 2)
    assert bool((out[empty] == 0).all()), "a row that sees no key must give out = 0"
    dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
    hip_attn_backward(do, q, k, v, want["out"].to(q.dtype), want["lse"].float(), dq, dk, dv, 0.0, None, causal)
    assert _C.last_launch_kinds() == KINDS["bwd"]
    _check(dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv), want, dt, Sq, Sk, Hq // Hkv)


def test_running_max_jumps(dev):
    """test_gpu_parity.py::test_softmax_rescale_branch's inputs: one key per 64-key tile is aligned with row 300, so its maximum
    grows tile after tile while the other rows of its block keep theirs."""
    from yunchang_amd.kernels import hip_attn_forward
    dt, S = "bfloat16", 512
    q, k, v, do = _inputs(1, S, S, 1, 1, dt, dev, seed=3)
    k = k * 0.125
    for t in range(S // 64):
        k[0, 64 * t + 5, 0] = q[0, 300, 0] * (0.5 + 0.25 * t)
    out, lse = hip_attn_forward(q, k, v, causal=False)
    _check(dict(out=out, lse=lse), _ref(q, k, v, do, False), dt, S, S, 1)


def _poisoned_view(t, fill=float("nan")):
    """`t`'s values as a strided view (row pitch and head pitch padded, 16-byte aligned offset) into memory full of NaN"""
    B, S, H, D = t.shape
    big = torch.full((B, S + 2, H + 1, D + 8), fill, dtype=t.dtype, device=t.device)
    view = big[:, 1:S + 1, :H, 8:]
    view.copy_(t)
    return view


def test_strided_views_ring_step_and_gradient_forms(dev):
    """One ragged GQA case, every tensor a strided view into poisoned memory: a two-call ring step on the C ABI (the keys in two
    halves: acc, merge_in, a final range on the second call), then the fp32, accumulating and 16-bit gradient forms."""
    from yunchang_amd import _C
    dt, (B, Sq, Sk, Hq, Hkv) = "bfloat16", (1, 300, 2 * 168, 4, 2)
    q, k, v, do = _inputs(B, Sq, Sk, Hq, Hkv, dt, dev, seed=5)
    want = _ref(q, k, v, do, False)
    pq, pk, pv, pdo = (_poisoned_view(t) for t in (q, k, v, do))
    scale, h = DQK ** -0.5, Sk // 2
    out = _poisoned_view(torch.zeros_like(do))
    acc = _poisoned_view(torch.zeros(B, Sq, Hq, DV, dtype=torch.float32, device=dev))
    lse = torch.empty(B, Hq, Sq, dtype=torch.float32, device=dev)
    _C.flash_fwd(pq, pk[:, :h], pv[:, :h], scale, False, lse, out=out, acc=acc, final_begin=0, final_end=0)
    _C.flash_fwd(pq, pk[:, h:], pv[:, h:], scale, False, lse, out=out, acc=acc, merge_in=True, final_begin=100, final_end=Sq)
    assert _C.last_launch_kinds() == KINDS["fwd"]
    _check(dict(out=out[:, 100:], lse=lse), dict(out=want["out"][:, 100:], lse=want["lse"]), dt, Sq, Sk, 2, "ring step ")
    assert_close(acc[:, :100].double(), want["out"][:, :100], *TOL[dt]["out"], "ring step acc")
    delta = torch.empty_like(lse)
    o16 = want["out"].to(q.dtype)
    _C.bwd_delta(pdo, _poisoned_view(o16), delta)
    g32 = [_poisoned_view(torch.zeros(t.shape, dtype=torch.float32, device=dev)) for t in (q, k, v)]
    g16 = [_poisoned_view(torch.zeros_like(t)) for t in (q, k, v)]
    lse_ref = want["lse"].float()
    _C.flash_bwd(pdo, pq, pk, pv, lse_ref, delta, *g32, scale, False)                                  # fp32, written
    _check(dict(zip(("dq", "dk", "dv"), g32)), want, dt, Sq, Sk, 2, "fp32 ")
    _C.flash_bwd(pdo, pq, pk, pv, lse_ref, delta, *g32, scale, False, True, True, True)                # fp32, accumulated
    _check(dict(zip(("dq", "dk", "dv"), (t / 2 for t in g32))), want, dt, Sq, Sk, 2, "accumulated ")
    _C.flash_bwd(pdo, pq, pk, pv, lse_ref, delta, *g32, scale, False, True, True, True, *g16)          # 16-bit: fp32 + new, rounded once
    _check(dict(zip(("dq", "dk", "dv"), (t.double() / 3 for t in g16))), want, dt, Sq, Sk, 2, "16-bit ")
    assert _C.last_launch_kinds() == KINDS["bwd"]


def test_multi_pass_launch_every_element(dev):
    """More items than resident workgroups in each kernel: 2 x 16 x 9 = 288 forward items, 576 dQ items, 2 x 8 x 18 = 288 dK/dV
    items of two query heads each on 256 CUs (the second pass of ItemWalk: LDS buffers, accumulators and row statistics reused).
    Every element against fp64 torch on the device, head by head, and the persistent launch bit for bit against
    USP_LAUNCH_INTERLEAVE (one workgroup per item)."""
    from yunchang_amd import _C
    dt, (B, S, Hq, Hkv) = "bfloat16", (2, 2304, 16, 8)
    q, k, v, do = _inputs(B, S, S, Hq, Hkv, dt, dev, seed=20)
    want = {n: [] for n in ("out", "lse", "dq", "dk", "dv")}
    for hk in range(Hkv):
        r = _ref(q[:, :, 2 * hk:2 * hk + 2], k[:, :, hk:hk + 1], v[:, :, hk:hk + 1], do[:, :, 2 * hk:2 * hk + 2], True)
        for n in want:
            want[n].append(r[n])
    want = {n: torch.cat(ts, dim=1 if n == "lse" else 2) for n, ts in want.items()}
    o16, lse_ref = want["out"].to(q.dtype), want["lse"].float()
    runs = []
    for interleave in (False, True):
        out, lse, delta = torch.empty_like(do), torch.empty_like(lse_ref), torch.empty_like(lse_ref)
        _C.flash_fwd(q, k, v, DQK ** -0.5, True, lse, out=out, interleave=interleave)
        _C.bwd_delta(do, o16, delta)
        dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
        _C.flash_bwd(do, q, k, v, lse_ref, delta, None, None, None, DQK ** -0.5, True, dq16=dq, dk16=dk, dv16=dv, interleave=interleave)
        runs.append(dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv))
    for n in want:
        assert torch.equal(runs[0][n], runs[1][n]), f"{n}: the persistent launch differs from one workgroup per item"
    _check(runs[0], want, dt, S, S, 2, "multi-pass ")


def test_autograd_without_host_sync(dev):
    from yunchang_amd.kernels import hip_attn_func
    dt, (B, Sq, Sk, Hq, Hkv) = "bfloat16", (1, 200, 264, 4, 2)
    q, k, v, do = _inputs(B, Sq, Sk, Hq, Hkv, dt, dev, seed=40)
    want = _ref(q, k, v, do, True)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = hip_attn_func(q, k, v, causal=True)
        out.backward(do)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert v.grad.shape == v.shape and out.shape == (B, Sq, Hq, DV)
    _check(dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad), want, dt, Sq, Sk, 2)


@pytest.fixture(scope="module")
def nccl_single():
    import os
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29748")
    own = not dist.is_initialized()
    if own:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    yield dist
    if own:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("ud,rd,impl", [(1, 2, "basic"), (1, 2, "zigzag"), (2, 1, "basic"), (2, 2, "basic")])
def test_rings_and_exchanges_on_the_virtual_grid(dev, nccl_single, monkeypatch, ud, rd, impl):
    """What LongContextAttention.forward runs at (192, 128) -- three separate Ulysses exchanges, the ring, the exchange back, and the
    same in reverse for the gradients -- on a virtual ud x rd grid with S_local = 192: the basic and the zigzag ring at degree 2,
    Ulysses at degree 2, the 2 x 2 grid, against the single-device fp64 result.  (The Functions are driven by hand, forward then
    backward on the rank's own thread, as the virtual grid needs it.)"""
    from oracle import usp_oracle as O
    from virtual_grid import Ctx, VirtualGrid, patch_dist, run_grid
    import yunchang_amd.comm.all_to_all as A
    import yunchang_amd.comm.relay_exchange as RX
    from yunchang_amd.ring.ring_flash_attn import ring_flash_attn_backward, ring_flash_attn_forward
    from yunchang_amd.ring.zigzag_ring_flash_attn import zigzag_ring_flash_attn_backward, zigzag_ring_flash_attn_forward
    fwd, bwd = {"basic": (ring_flash_attn_forward, ring_flash_attn_backward),
                "zigzag": (zigzag_ring_flash_attn_forward, zigzag_ring_flash_attn_backward)}[impl]
    dt, (Hq, Hkv), ws = "bfloat16", (4, 2), ud * rd
    S = 192 * ws
    full = _inputs(1, S, S, Hq, Hkv, dt, dev, seed=60)
    want = _ref(*full, True)
    grid = VirtualGrid(ud, rd, nccl_single)
    patch_dist(monkeypatch, grid)
    monkeypatch.setitem(RX._OVERRIDE, "relay", False)
    shard = lambda x, r: torch.from_numpy(np.ascontiguousarray(O.EXTRACT[impl](x.float().cpu().numpy(), r, ws, rd, ud))).to(x.dtype).to(dev)
    loc = [[shard(x, r) for x in full] for r in range(ws)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(ws)]
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        upg, rpg = grid.groups_of(r)
        with torch.cuda.stream(streams[r]):
            q, k, v, do = loc[r]
            cx = [Ctx() for _ in range(4)]
            if ud > 1:          # sequence shards -> head shards, q | k | v each at its own width
                q = A.SeqAllToAll4D.forward(cx[0], upg, q, 2, 1, False, False)
                k = A.SeqAllToAll4DKV.forward(cx[1], upg, k, 2, 1, False, False)
                v = A.SeqAllToAll4DKV.forward(cx[2], upg, v, 2, 1, False, False)
            out, lse = fwd(rpg, q, k, v, softmax_scale=DQK ** -0.5, causal=True)
            ctx_out = out
            if ud > 1:
                out = A.SeqAllToAll4D.forward(cx[3], upg, out, 1, 2, False, False)
                do = A.SeqAllToAll4D.backward(cx[3], do)[1]
            dq, dk, dv = bwd(rpg, do.contiguous(), q, k, v, ctx_out, lse, softmax_scale=DQK ** -0.5, causal=True)[:3]
            if ud > 1:
                dq = A.SeqAllToAll4D.backward(cx[0], dq)[1]
                dk = A.SeqAllToAll4DKV.backward(cx[1], dk)[1]
                dv = A.SeqAllToAll4DKV.backward(cx[2], dv)[1]
            return dict(out=out, dq=dq, dk=dk, dv=dv)

    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    for r in range(ws):
        assert res[r]["out"].shape[-1] == DV and res[r]["dv"].shape[-1] == DV and res[r]["dk"].shape[-1] == DQK
        _check(res[r], {n: shard(want[n], r).double() for n in res[r]}, dt, S, S, Hq // Hkv, f"{ud}x{rd} {impl} rank {r} ")
