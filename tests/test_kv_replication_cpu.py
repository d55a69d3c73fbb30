"""Ulysses degrees larger than the KV head count (Hkv < P, P % Hkv == 0): every rank gets a replica of KV head p // r
(r = P / Hkv) beside its Hq/P query heads, and the sequence owners sum the r dK/dV partials of each head in fp32, in
ascending Ulysses rank order (comm/all_to_all.py:kv_replicas).  CPU: gloo ranks with the fp64 oracle as the block backend;
truth is exact attention and its gradients on the unsharded tensors."""
import os

import numpy as np
import pytest
import torch

from dist_util import run_distributed
from golden_util import TOL, grad_tol

TOL_OUT = TOL["bfloat16"]["out"][0]
TOL_GRAD = grad_tol("bfloat16", 8)[0]


def _setup(rank, ws, ud, rd, backend=None):
    import yunchang_amd as Y
    from yunchang_amd.kernels import set_block_backend
    from oracle_backend import OracleBlockBackend
    set_block_backend(backend or OracleBlockBackend())
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    return Y


def _inputs(ws, Hq, Hkv, B=2, D=32, rows=32, seed=0):
    torch.manual_seed(seed)
    S = rows * ws
    return tuple(torch.randn(B, S, h, D).to(torch.bfloat16) for h in (Hq, Hkv, Hkv, Hq))


def _truth(Y, rank, ws, ud, rd, impl, q, k, v, do, window=None):
    from oracle import usp_oracle as O
    ext = Y.EXTRACT_FUNC_DICT[impl]
    qn, kn, vn, don = (t.float().numpy().astype(np.float64) for t in (q, k, v, do))
    kw = {} if window is None else {"window": window}
    ro, rl = O.attention_ref(qn, kn, vn, causal=True, **kw)
    return [ext(torch.from_numpy(np.ascontiguousarray(t)), rank, world_size=ws, rd=rd, ud=ud).float()
            for t in (ro,) + tuple(O.block_bwd(don, qn, kn, vn, ro, rl, None, True, **kw))]


def _run(Y, layer, rank, ws, ud, rd, impl, q, k, v, do, env=None, **call):
    ext = Y.EXTRACT_FUNC_DICT[impl]
    lq, lk, lv, ldo = (ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in (q, k, v, do))
    for t in (lq, lk, lv):
        t.requires_grad_(True)
    env = env or {}
    os.environ.update(env)
    try:
        out = layer(lq, lk, lv, causal=True, **call)
        out.backward(ldo)
    finally:
        for key in env:
            del os.environ[key]
    return [t.detach().float() for t in (out, lq.grad, lk.grad, lv.grad)]


def _right(got, truth):
    return all(torch.allclose(a, t, atol=tol, rtol=tol) for a, t, tol in zip(got, truth, (TOL_OUT,) + (TOL_GRAD,) * 3))


def _errs(got, truth):
    return [round(float((a - t).abs().max()), 4) for a, t in zip(got, truth)]


# ---- the layers on the grids -------------------------------------------------------------------------------------------------
def _grid_worker(rank, ws, ud, rd, impl, Hq, Hkv):
    Y = _setup(rank, ws, ud, rd)
    import yunchang_amd.comm.all_to_all as A
    import yunchang_amd.hybrid.async_attn_layer as AL
    assert A.kv_replicas(Hkv, ud) == ud // Hkv > 1
    q, k, v, do = _inputs(ws, Hq, Hkv)
    truth = _truth(Y, rank, ws, ud, rd, impl, q, k, v, do)
    # at ulysses degree 2 beside a zigzag ring the self-chunk start, the row-chunked tails and dq-first are defaults; the tiny
    # problem would size the tails away, so their piece count is pinned
    AL._COMM_OVERRIDE.update(tails="2")
    seen = {"self": 0, "tails": 0, "sum": 0}
    views, rows, sums = AL._self_views, A.pack_seq_rows, A._sum_rows

    def count(key, fn):
        def wrapped(*a, **kw):
            seen[key] += 1
            return fn(*a, **kw)
        return wrapped
    AL._self_views, A.pack_seq_rows, A._sum_rows = count("self", views), count("tails", rows), count("sum", sums)
    layers = [("packed", Y.LongContextAttention(ring_impl_type=impl), None),
              ("async", Y.AsyncLongContextAttention(ring_impl_type=impl), None),
              ("three-exchanges", Y.LongContextAttention(ring_impl_type=impl), {"USP_PACK_QKV": "0"})]
    if rd == 1:
        layers.append(("ulysses", Y.UlyssesAttention(Y.PROCESS_GROUP.ULYSSES_PG, attn_type=Y.AttnType.HIP), None))
    res = {}
    try:
        for name, layer, env in layers:
            got = _run(Y, layer, rank, ws, ud, rd, impl, q, k, v, do, env)
            res[name] = (_right(got, truth), _errs(got, truth))
    finally:
        AL._self_views, A.pack_seq_rows, A._sum_rows = views, rows, sums
        AL._COMM_OVERRIDE.clear()
    return res, seen


GRIDS = [(2, 2, 1, "basic", 4, 1), (4, 4, 1, "basic", 8, 2), (4, 4, 1, "basic", 4, 1),
         (8, 8, 1, "basic", 32, 4),            # the target shape's heads (H32 / Hkv4) as pure Ulysses 8
         (4, 2, 2, "zigzag", 4, 1), (8, 2, 4, "zigzag", 8, 1), (8, 4, 2, "zigzag", 8, 2), (4, 2, 2, "strip", 4, 1)]


@pytest.mark.parametrize("ws,ud,rd,impl,Hq,Hkv", GRIDS, ids=lambda x: str(x))
def test_layers_with_kv_heads_shared_by_ulysses_ranks_match_exact_attention(ws, ud, rd, impl, Hq, Hkv):
    """out, dq, dk, dv of LongContextAttention (packed default), AsyncLongContextAttention, the reference's three exchanges
    (USP_PACK_QKV=0) and, at ring degree 1, UlyssesAttention equal exact attention within the bf16 tolerances."""
    for rank, (res, seen) in enumerate(run_distributed(_grid_worker, ws, ud, rd, impl, Hq, Hkv)):
        for name, (ok, errs) in res.items():
            assert ok, (rank, name, errs)
        assert seen["sum"] == 2 * len(res), seen               # dk and dv of every layer were summed over the replicas
        if (ud, impl) == (2, "zigzag") and rd > 1:              # the 2 x 4 grid's defaults ran on the replicated head
            assert seen["self"] > 0 and seen["tails"] > 0, seen


# ---- softcap, a sliding window, the relayed pair exchange -------------------------------------------------------------------
def _softcap_worker(rank, ws, ud, rd, impl, Hq, Hkv):
    from test_softcap_cpu import CAP, _softcap_backend, make_case, np64, ref_bwd, ref_fwd
    be = _softcap_backend()
    Y = _setup(rank, ws, ud, rd, be)
    B, S, D = 1, 64, 32
    q, k, v, do = make_case(B, S, S, Hq, Hkv, D, seed=1)
    scale = D ** -0.5
    qn, kn, vn, don = (np64(t) for t in (q, k, v, do))
    ro, _ = ref_fwd(qn, kn, vn, scale, CAP, True)
    ext = Y.EXTRACT_FUNC_DICT[impl]
    truth = [ext(torch.from_numpy(np.ascontiguousarray(t)), rank, world_size=ws, rd=rd, ud=ud).float()
             for t in (ro,) + tuple(ref_bwd(don, qn, kn, vn, scale, CAP, True))]
    got = _run(Y, Y.LongContextAttention(ring_impl_type=impl), rank, ws, ud, rd, impl, q, k, v, do, softcap=CAP)
    return _right(got, truth), _errs(got, truth), sorted({c[0] for c in be.calls})


def test_softcap_with_shared_kv_heads():
    for ok, errs, kinds in run_distributed(_softcap_worker, 4, 2, 2, "zigzag", 4, 1):
        assert ok, errs
        assert kinds == ["bwd-softcap", "fwd-softcap"], kinds


def _window_worker(rank, ws, ud, Hq, Hkv):
    Y = _setup(rank, ws, ud, 1)
    win = (40, 0)
    q, k, v, do = _inputs(ws, Hq, Hkv, rows=64)
    truth = _truth(Y, rank, ws, ud, 1, "basic", q, k, v, do, window=win)
    res = []
    for layer in (Y.LongContextAttention(ring_impl_type="basic"),
                  Y.UlyssesAttention(Y.PROCESS_GROUP.ULYSSES_PG, attn_type=Y.AttnType.HIP)):
        got = _run(Y, layer, rank, ws, ud, 1, "basic", q, k, v, do, window_size=win)
        res.append((_right(got, truth), _errs(got, truth)))
    return res


def test_sliding_window_with_shared_kv_heads():
    """A window at ring degree 1 takes the reference's structure (three exchanges): k and v through the KV form."""
    for res in run_distributed(_window_worker, 4, 4, 8, 2):
        for ok, errs in res:
            assert ok, errs


def _relay_worker(rank, ws, ud, rd, Hq, Hkv):
    Y = _setup(rank, ws, ud, rd)
    import yunchang_amd.comm.relay_exchange as RX
    q, k, v, do = _inputs(ws, Hq, Hkv)
    truth = _truth(Y, rank, ws, ud, rd, "zigzag", q, k, v, do)
    res, used = [], []
    applicable = RX.applicable
    RX.applicable = lambda send, group: used.append(applicable(send, group)) or used[-1]
    try:
        for env in ({"USP_EXCHANGE_RELAY": "0"}, {"USP_EXCHANGE_RELAY": "1"}):
            res.append(_run(Y, Y.LongContextAttention(ring_impl_type="zigzag"), rank, ws, ud, rd, "zigzag", q, k, v, do, env))
    finally:
        RX.applicable = applicable
    return all(torch.equal(a, b) for a, b in zip(*res)), _right(res[1], truth), any(used)


def test_relayed_pair_exchange_with_shared_kv_heads():
    """USP_EXCHANGE_RELAY=1 at ulysses degree 2 (the pair's exchange striped over the other ranks): bit-identical to the
    direct exchange and right."""
    for same, right, used in run_distributed(_relay_worker, 4, 2, 2, 4, 1):
        assert same and right and used


# ---- determinism, the r = 1 path, refusals -----------------------------------------------------------------------------------
def _repeat_worker(rank, ws, ud, rd, impl, Hq, Hkv):
    Y = _setup(rank, ws, ud, rd)
    q, k, v, do = _inputs(ws, Hq, Hkv)
    layer = Y.LongContextAttention(ring_impl_type=impl)
    a = _run(Y, layer, rank, ws, ud, rd, impl, q, k, v, do)
    b = _run(Y, layer, rank, ws, ud, rd, impl, q, k, v, do)
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("ws,ud,rd,impl,Hq,Hkv", [(4, 4, 1, "basic", 8, 1), (8, 2, 4, "zigzag", 8, 1)])
def test_two_backward_passes_are_bit_identical(ws, ud, rd, impl, Hq, Hkv):
    assert all(run_distributed(_repeat_worker, ws, ud, rd, impl, Hq, Hkv))


def _divisible_worker(rank, ws, ud, rd, impl, Hq, Hkv):
    Y = _setup(rank, ws, ud, rd)
    import yunchang_amd.comm.all_to_all as A

    def refuse(*a, **kw):
        raise AssertionError("the replica path ran at Hkv % P == 0")
    saved = A._sum_rows, A.pack_kv_replicated
    A._sum_rows = A.pack_kv_replicated = refuse
    try:
        q, k, v, do = _inputs(ws, Hq, Hkv)
        truth = _truth(Y, rank, ws, ud, rd, impl, q, k, v, do)
        layers = [(Y.LongContextAttention(ring_impl_type=impl), None), (Y.AsyncLongContextAttention(ring_impl_type=impl), None),
                  (Y.LongContextAttention(ring_impl_type=impl), {"USP_PACK_QKV": "0"})]
        if rd == 1:
            layers.append((Y.UlyssesAttention(Y.PROCESS_GROUP.ULYSSES_PG, attn_type=Y.AttnType.HIP), None))
        return all(_right(_run(Y, layer, rank, ws, ud, rd, impl, q, k, v, do, env), truth) for layer, env in layers)
    finally:
        A._sum_rows, A.pack_kv_replicated = saved


@pytest.mark.parametrize("ws,ud,rd,impl,Hq,Hkv", [(4, 2, 2, "zigzag", 8, 4), (4, 4, 1, "basic", 8, 4)])
def test_divisible_kv_heads_never_reach_the_replica_path(ws, ud, rd, impl, Hq, Hkv):
    assert all(run_distributed(_divisible_worker, ws, ud, rd, impl, Hq, Hkv))


def _refusal_worker(rank, ws, Hq, Hkv):
    Y = _setup(rank, ws, ws, 1)
    q, k, v, do = _inputs(ws, Hq, Hkv)
    out = []
    for layer, env in ((Y.LongContextAttention(ring_impl_type="basic"), None),
                       (Y.LongContextAttention(ring_impl_type="basic"), {"USP_PACK_QKV": "0"}),
                       (Y.AsyncLongContextAttention(ring_impl_type="basic"), None),
                       (Y.UlyssesAttention(Y.PROCESS_GROUP.ULYSSES_PG, attn_type=Y.AttnType.HIP), None)):
        try:
            _run(Y, layer, rank, ws, ws, 1, "basic", q, k, v, do, env)
            out.append("ran")
        except AssertionError:
            out.append("AssertionError")
    return out


@pytest.mark.parametrize("Hq,Hkv", [(12, 3),      # Hkv < P, P % Hkv != 0
                                    (6, 2)])      # Hq % P != 0
def test_unserved_head_counts_still_raise(Hq, Hkv):
    for res in run_distributed(_refusal_worker, 4, Hq, Hkv):
        assert res == ["AssertionError"] * 4, res


def test_groups_with_shared_kv_heads():
    import yunchang_amd.hybrid.async_attn_layer as AL
    assert AL._groups(32, 4, 8) == (1, 1, 4)
    assert AL._groups(8, 1, 2, B=1, S=1 << 16) == (1, 1, 4)
    assert AL._groups(32, 8, 4) == (2, 1, 4)                      # r = 1: as before
    for bad in ((6, 6, 4), (12, 3, 4), (6, 2, 4), (8, 6, 4)):
        with pytest.raises(AssertionError):
            AL._groups(*bad)


def test_kv_replicas_map():
    import yunchang_amd.comm.all_to_all as A
    assert [A.kv_replicas(h, 8) for h in (1, 2, 3, 4, 8, 16, 12)] == [8, 4, 0, 2, 1, 1, 0]
    assert A.kv_replicas(1, 1) == 1


def test_link_bound_counts_the_replicated_kv_bytes(monkeypatch):
    """With Hkv = 1 at P = 8 a rank sends its one KV head to all 8 ranks: its exchange moves 2 Hq + 16 head rows, not 2 Hq + 2."""
    import yunchang_amd.hybrid.async_attn_layer as AL
    monkeypatch.setattr(AL, "_KERNEL_FLOPS_PER_S", 1e15)
    B, S, D, Hq = 1, 1 << 14, 128, 16
    flops = 4.0 * B * (Hq // 8) * S * S * D * 0.5
    t_attn = flops / 1e15
    for Hkv, heads in ((1, 2 * Hq + 16), (8, 2 * Hq + 16), (16, 2 * Hq + 32)):
        t_comm = lambda rate: B * (S // 8) * heads * D * 2 / 8 / rate
        rate = t_comm(1.0) / (0.5 * t_attn)                     # the exchange exactly half as long as the attention
        monkeypatch.setattr(AL, "_LINK_BYTES_PER_S", rate * 0.99)
        assert AL._link_bound(Hq, Hkv, 8, B, S, D, 2, 1, True)
        monkeypatch.setattr(AL, "_LINK_BYTES_PER_S", rate * 1.01)
        assert not AL._link_bound(Hq, Hkv, 8, B, S, D, 2, 1, True)


# ---- the host forms of the pack and the reduce ---------------------------------------------------------------------------------
@pytest.mark.parametrize("P,Hkv,Ht,h0,dtype", [(8, 4, 6, 4, torch.bfloat16), (4, 1, 3, 1, torch.float16),
                                               (8, 1, 2, 0, torch.bfloat16)])
def test_host_pack_and_reduce(P, Hkv, Ht, h0, dtype):
    """pack_kv_replicated puts KV head p // r in chunk p; unpack_kv_sum equals a sequential fp32 sum over the r chunks of a
    head in ascending rank order, rounded once (and differs from a bf16/fp16 running sum)."""
    import yunchang_amd.comm.all_to_all as A
    r = A.kv_replicas(Hkv, P)
    B, Sl, D = 2, 5, 16
    g = torch.Generator().manual_seed(P * 10 + Hkv)
    x = (torch.randn(B, Sl, Hkv, D, generator=g) * 3).to(dtype)
    send = torch.full((P, Sl, B, Ht, D), float("nan"), dtype=dtype)
    A.pack_kv_replicated(send, h0, x, r)
    for p in range(P):
        assert torch.equal(send[p, :, :, h0], x[:, :, p // r].transpose(0, 1))
    others = [h for h in range(Ht) if h != h0]
    assert torch.isnan(send[:, :, :, others].float()).all()
    recv = (torch.randn(P, Sl, B, Ht, D, generator=g) * 100).to(dtype)
    dst = torch.full((B, Sl, Hkv, D), float("nan"), dtype=dtype)
    A.unpack_kv_sum(recv, dst, h0, r)
    want = torch.empty_like(dst)
    for h in range(Hkv):
        acc = torch.zeros(Sl, B, D, dtype=torch.float32)
        for t in range(r):
            acc = acc + recv[h * r + t, :, :, h0].float()
        want[:, :, h] = acc.to(dtype).transpose(0, 1)
    assert torch.equal(dst, want)
    if r > 2:
        running = recv[0, :, :, h0].clone()
        for t in range(1, r):
            running = running + recv[t, :, :, h0]
        assert not torch.equal(running.transpose(0, 1), want[:, :, 0])   # the fp32 sum is what the test pins


def test_sum_rows_export_validates_before_any_launch():
    """usp_sum_rows (include/usp_hip.h) refuses null pointers, r < 1, non-positive sizes and bad dtypes with USP_EINVAL and
    16-byte misalignment with USP_EUNSUPPORTED, before it touches the device (safe without a GPU)."""
    import ctypes
    from yunchang_amd import _C
    L = _C.load()
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 15) & ~15
    ok = [0, a, a + 1024, 128, 2, 256, 4, 1, 1, 128, 0, 0, 128, 0, 0, None]
    for i, val, code in ((1, None, -1), (2, None, -1), (3, 0, -1), (4, 0, -1), (4, -3, -1), (6, 0, -1), (8, -1, -1),
                         (0, 2, -1), (3, 24, -2), (5, 40, -2), (10, 8, -2), (14, 4, -2), (1, a + 2, -2), (2, a + 8, -2)):
        args = list(ok)
        args[i] = val
        assert L.usp_sum_rows(*args) == code, (i, val)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        _C.sum_rows(torch.zeros(64, dtype=torch.bfloat16), torch.zeros(128, dtype=torch.bfloat16), 128, 2, 128, [1], [0], [0])


def test_host_reduce_refuses_what_the_device_refuses():
    import yunchang_amd.comm.all_to_all as A
    recv = torch.zeros(4, 3, 1, 2, 12, dtype=torch.bfloat16)                 # rows of 24 bytes
    dst = torch.zeros(1, 3, 2, 12, dtype=torch.bfloat16)
    with pytest.raises(AssertionError):
        A.unpack_kv_sum(recv, dst, 0, 2)
