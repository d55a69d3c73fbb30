"""Ulysses degrees larger than the KV head count on the device: the r-term row sum behind the dK/dV return
(usp_sum_rows) bit for bit against a sequential fp32 sum, the layers on the real kernels with several processes sharing
cuda:0 over gloo, and the target shape's heads (H32 / Hkv4 D128) as pure Ulysses 8 at S = 16384 on the RCCL virtual grid."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dist_util import run_distributed

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _seq_sum(terms, dtype):
    """acc = 0; for t: acc = acc + x_t.float(); -> dtype: the sum the kernel must reproduce bit for bit."""
    acc = torch.zeros(terms[0].shape, dtype=torch.float32, device=terms[0].device)
    for x in terms:
        acc = acc + x.float()
    return acc.to(dtype)


# ---- usp_sum_rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("r", [1, 2, 4, 8])
def test_sum_rows_is_a_sequential_fp32_sum(dtype, r):
    """Contiguous rows (an odd row count) and the exchange's strided layout (receive buffer (P, S/P, B, Ht, D) -> one head
    of (B, S/P, Hkv, D)), each written into a NaN canary: the rows it owns equal the sequential sum bit for bit, every other
    element stays NaN."""
    from yunchang_amd import _C
    import yunchang_amd.comm.all_to_all as A
    torch.cuda.set_device(DEV)
    g = torch.Generator(device=DEV).manual_seed(r)
    # (1) plain rows: 1001 rows of 96 elements, terms `term` elements apart
    rows, n, term = 1001, 96, 1001 * 96 + 64
    src = (torch.randn(r * term, device=DEV, generator=g) * 50).to(dtype)
    canvas = torch.full((rows + 2, n + 16), float("nan"), dtype=dtype, device=DEV)
    dst = canvas[1:rows + 1, 8:8 + n]
    es = src.element_size()
    _C.sum_rows(dst, src, n * es, r, term * es, [rows], [dst.stride(0) * es], [n * es])
    torch.cuda.synchronize()
    want = _seq_sum([src[t * term:t * term + rows * n].view(rows, n) for t in range(r)], dtype)
    assert torch.equal(dst, want)
    keep = torch.ones(canvas.shape, dtype=torch.bool, device=DEV)
    keep[1:rows + 1, 8:8 + n] = False
    assert torch.isnan(canvas[keep].float()).all()
    # (2) the exchange's layout: P = r Hkv chunks of (S/P, B, Ht, D), the gradient at head h0 of every chunk
    Hkv, Sl, B, Ht, D, h0 = 3, 37, 2, 5, 128, 2
    P = r * Hkv
    recv = (torch.randn(P, Sl, B, Ht, D, device=DEV, generator=g) * 50).to(dtype)
    out = torch.full((B, Sl, Hkv + 1, D), float("nan"), dtype=dtype, device=DEV)
    c = Sl * B * Ht * D
    if r > 1:
        A.unpack_kv_sum(recv, out[:, :, :Hkv], h0, r)
    else:                                   # (r = 1 never reaches the kernel in the layers; the kernel serves it)
        _C.sum_rows(out, recv[0, 0, 0, h0], D * es, 1, c * es, [Hkv, Sl, B],
                    [D * es, (Hkv + 1) * D * es, Sl * (Hkv + 1) * D * es], [c * es, B * Ht * D * es, Ht * D * es])
    torch.cuda.synchronize()
    for h in range(Hkv):
        want = _seq_sum([recv[h * r + t, :, :, h0] for t in range(r)], dtype).transpose(0, 1)
        assert torch.equal(out[:, :, h], want), h
    assert torch.isnan(out[:, :, Hkv].float()).all()


def test_sum_rows_refuses_bad_arguments_without_a_launch():
    from yunchang_amd import _C
    L = _C.load()
    torch.cuda.set_device(DEV)
    src = torch.ones(4096, dtype=torch.bfloat16, device=DEV)
    dst = torch.full((1024,), float("nan"), dtype=torch.bfloat16, device=DEV)
    d, s = ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    # 16 rows of 128 bytes (all of dst), two terms 2048 bytes apart: dst = 1 + 1
    ok = [0, d, s, 128, 2, 2048, 16, 1, 1, 128, 0, 0, 128, 0, 0, st]
    bad = {-1: [(1, None), (2, None), (3, 0), (4, 0), (6, 0), (7, -1), (0, 7)],
           -2: [(3, 120), (5, 1000), (9, 136), (12, 72), (1, ctypes.c_void_p(dst.data_ptr() + 2)),
                (2, ctypes.c_void_p(src.data_ptr() + 8))]}
    torch.cuda.synchronize()
    for code, cases in bad.items():
        for i, val in cases:
            args = list(ok)
            args[i] = val
            assert L.usp_sum_rows(*args) == code, (i, val)
    torch.cuda.synchronize()
    assert torch.isnan(dst.float()).all()                    # nothing ran
    assert L.usp_sum_rows(*ok) == 0
    torch.cuda.synchronize()
    assert bool((dst.float() == 2.0).all())


# ---- the layers on the real kernels: processes sharing cuda:0 over gloo --------------------------------------------------------
def _layer_worker(rank, ws, cases):
    import yunchang_amd as Y
    import yunchang_amd.comm.all_to_all as A
    from oracle import usp_oracle as O
    from test_gpu_multiproc import _order_p2p_like_rccl
    from yunchang_amd.kernels import get_block_backend
    _order_p2p_like_rccl()
    assert get_block_backend().name == "hip"
    torch.cuda.set_device(DEV)
    res = []
    for ud, rd, impl, Hq, Hkv, D in cases:
        Y.set_seq_parallel_pg(ud, rd, rank, ws)
        assert A.kv_replicas(Hkv, ud) > 1
        torch.manual_seed(0)
        B, S = 1, 128 * ws
        q, k, v, do = (torch.randn(B, S, h, D).to(torch.bfloat16) for h in (Hq, Hkv, Hkv, Hq))
        ext = Y.EXTRACT_FUNC_DICT[impl]
        qn, kn, vn, don = (t.float().numpy().astype(np.float64) for t in (q, k, v, do))
        ro, rl = O.attention_ref(qn, kn, vn, causal=True)
        truth = [ext(torch.from_numpy(np.ascontiguousarray(t)), rank, world_size=ws, rd=rd, ud=ud).float()
                 for t in (ro,) + tuple(O.block_bwd(don, qn, kn, vn, ro, rl, None, True))]
        layers = [("packed", Y.LongContextAttention(ring_impl_type=impl, attn_type=Y.AttnType.HIP), None),
                  ("async", Y.AsyncLongContextAttention(ring_impl_type=impl), None),
                  ("three-exchanges", Y.LongContextAttention(ring_impl_type=impl, attn_type=Y.AttnType.HIP), {"USP_PACK_QKV": "0"})]
        if rd == 1:
            layers.append(("ulysses", Y.UlyssesAttention(Y.PROCESS_GROUP.ULYSSES_PG, attn_type=Y.AttnType.HIP), None))
        for name, layer, env in layers:
            runs = []
            for _ in range(2):                                # twice: bit-identical, buffers reusable
                lq, lk, lv, ldo = (ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone().to(DEV) for t in (q, k, v, do))
                for t in (lq, lk, lv):
                    t.requires_grad_(True)
                os.environ.update(env or {})
                try:
                    out = layer(lq, lk, lv, causal=True)
                    out.backward(ldo)
                finally:
                    for key in env or {}:
                        del os.environ[key]
                torch.cuda.synchronize()
                runs.append([t.detach().float().cpu() for t in (out, lq.grad, lk.grad, lv.grad)])
            errs = [round(float((a - t).abs().max()), 4) for a, t in zip(runs[0], truth)]
            same = all(torch.equal(a, b) for a, b in zip(*runs))
            ok = all(torch.allclose(a, t, atol=tol, rtol=tol) for a, t, tol in zip(runs[0], truth, (2e-2, 5e-2, 5e-2, 5e-2)))
            res.append(((ud, rd, impl, Hq, Hkv, name), ok, same, errs))
    return res


@pytest.mark.timeout(600)
@pytest.mark.parametrize("ws,cases", [(4, [(4, 1, "basic", 8, 2, 64), (4, 1, "basic", 4, 1, 128)]),
                                      (8, [(8, 1, "basic", 32, 4, 128), (2, 4, "zigzag", 8, 1, 128)])],
                         ids=["ws4_u4_hkv2_hkv1", "ws8_u8_h32kv4_and_u2r4_zigzag_mqa"])
def test_layers_with_shared_kv_heads_on_the_kernels(ws, cases):
    """ws 4: ulysses 4 with Hkv 2 and 1; ws 8: ulysses 8 with H32 / Hkv4 and ulysses 2 x zigzag ring 4 with MQA (the
    self-chunk start, tails and dq-first defaults): out, dq, dk, dv of every layer against fp64 exact attention, and two
    passes bit-identical."""
    for rank, res in enumerate(run_distributed(_layer_worker, ws, cases)):
        for case, ok, same, errs in res:
            assert ok and same, (rank, case, same, errs)


# ---- the target shape's heads as pure Ulysses 8, full size, every exchange a real RCCL call -----------------------------------
@pytest.fixture(scope="module")
def nccl_one():
    import torch.distributed as dist
    import yunchang_amd  # noqa: F401
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29747")
    own = not dist.is_initialized()
    if own:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    yield dist
    if own:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_ulysses8_h32_kv4_at_16k_on_a_virtual_grid(nccl_one, monkeypatch):
    """8 virtual ranks, ulysses 8 x ring 1, B1 S16384 H32/Hkv4 D128 bf16 causal, forward + backward through the layer's
    packed exchange (each KV head shared by two ranks), every exchange a real RCCL call: the shards put back together
    against the single-launch forward and against exact fp64 attention on sampled rows and key columns
    (bench.sampled_parity)."""
    import importlib.util
    from virtual_grid import Ctx, VirtualGrid, patch_dist, run_grid
    from yunchang_amd import _C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    cfg = dict(B=1, S=16384, Hq=32, Hkv=4, D=128)
    ud, rd, ws = 8, 1, 8
    q, k, v, do = b.make_global(cfg, DEV)
    loc = [[t.chunk(ws, dim=1)[r].contiguous() for t in (q, k, v, do)] for r in range(ws)]
    grid = VirtualGrid(ud, rd, nccl_one)
    AL = patch_dist(monkeypatch, grid)
    import yunchang_amd.comm.all_to_all as A
    sums = []
    real = A._sum_rows
    monkeypatch.setattr(A, "_sum_rows", lambda *a: (sums.append(a[3]), real(*a))[1])
    streams = [torch.cuda.Stream(device=DEV) for _ in range(ws)]
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(DEV)
        lq, lk, lv, ldo = loc[r]
        upg, rpg = grid.groups_of(r)
        ctx = Ctx()
        with torch.cuda.stream(streams[r]):
            out = AL._AsyncUSPFunc.forward(ctx, lq, lk, lv, None, True, upg, rpg, "basic", AL._MAX_GROUPS)
            grads = AL._AsyncUSPFunc.backward(ctx, ldo)[:3]
        return (out,) + tuple(grads), ctx.meta[6:9]

    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    assert {m for _, m in res} == {(1, 1, 4)}                     # one group, one KV head per rank, its 4 query heads
    assert sums == [2] * (2 * ws), sums                            # dk and dv of every rank: two replicas summed
    glob = [torch.cat([res[r][0][i] for r in range(ws)], dim=1) for i in range(4)]
    lse = torch.empty((1, cfg["Hq"], cfg["S"]), dtype=torch.float32, device=DEV)
    one = torch.empty_like(q)
    _C.flash_fwd(q, k, v, cfg["D"] ** -0.5, True, lse, one)
    d = (glob[0].float() - one.float()).abs()
    assert bool((d <= 2e-2 + 2e-2 * one.float().abs()).all()), float(d.max())
    err = b.sampled_parity(dict(q=q, k=k, v=v, do=do, out=glob[0], lse=lse, dq=glob[1], dk=glob[2], dv=glob[3]))["max_abs_err"]
    print("ulysses 8 x ring 1, H32/Hkv4, S16384: max abs errors vs fp64 samples:", err)
    g = cfg["Hq"] // cfg["Hkv"]
    assert err["out"] < 2e-2 and err["lse"] < 2e-3, err
    assert err["dq"] < 5e-2 and err["dk"] < 5e-2 * g ** 0.5 and err["dv"] < 5e-2 * g ** 0.5, err
