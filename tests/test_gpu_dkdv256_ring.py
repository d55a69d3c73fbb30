"""The 256-key-item dK/dV kernel across head switches and item switches: where its 3-deep LDS ring and its tile cursors stand.

`flash_bwd_dkdv64u_kernel` streams the Q / dO tiles of a head through three LDS buffers, keeps the buffer's byte offset and the
two LDS-DMA descriptors as running state (a descriptor is stepped in place, one tile per `dma_open`), and re-bases all of it when
the next head of the item or the next item of the persistent workgroup opens.  tests/test_gpu_dkdv256.py pins the arithmetic at
two to seven tiles per head; here the number of tiles a head streams takes every residue of the ring, and a workgroup runs
item after item.

Every case forces `family="row64"`, `only="dkdv"`, `dkdv_keys=256`, asserts `_C.last_dkdv_item_keys() == 256`, and compares
with np.array_equal against the 128-key kernel (`dkdv_keys=128`) on the same inputs and with golden_util.assert_close at
golden_util.grad_tol against oracle.usp_oracle.block_bwd.

- Ring position at every head switch: B1 Hq8 / Hkv2 D128, Sk = 256 (all four waves own keys), full mask, Sq in {64 .. 448}: a
  head streams 1 .. 7 tiles, so the ring stands at every residue when the next head opens; dkdv_heads in {1, 2, 4} (1, 2 or 4
  heads per item); bf16, and fp16 at Sq = 320, dkdv_heads = 2.
- Item after item in one workgroup: B2 Hq16 / Hkv16 D128 bf16 causal, Sq = Sk = 2304, dkdv_heads = 1: 2 x 16 x 9 = 288 items,
  more than the device has compute units (asserted), of 1 to 36 tiles.  Bit-identity is checked on every element; the oracle
  judges batch 0, heads 0 and 15 (G = 1: a head slices cleanly).  The forward results the launch needs (out for delta, lse)
  are the oracle's on those two heads and a float32 torch composition on the others.
"""
import functools

import numpy as np
import pytest
import torch

from golden_util import assert_close, grad_tol, round_to
from oracle import usp_oracle as O

pytestmark = pytest.mark.gpu

D = 128
SCALE = D ** -0.5


@pytest.fixture(scope="module")
def dev():
    from yunchang_amd import _C
    _C.load()
    return torch.device("cuda:0")


def _inputs(dt, B, Sq, Sk, HQ, HKV, seed):
    rs = np.random.RandomState(seed)
    q = round_to(rs.standard_normal((B, Sq, HQ, D)).astype(np.float32), dt)
    k = round_to(rs.standard_normal((B, Sk, HKV, D)).astype(np.float32), dt)
    v = round_to(rs.standard_normal((B, Sk, HKV, D)).astype(np.float32), dt)
    do = round_to(rs.standard_normal(q.shape).astype(np.float32), dt)
    return q, k, v, do


@functools.lru_cache(maxsize=None)
def ring_case(dt, Sq):
    """(q, k, v, do, o16, lse, reference dk, dv) of the head-switch shape: computed once per (dtype, Sq), shared, read-only."""
    q, k, v, do = _inputs(dt, 1, Sq, 256, 8, 2, 17)
    ro, rl = O.attention_ref(q, k, v, False, SCALE)
    o16 = round_to(ro.astype(np.float32), dt)
    _, rdk, rdv = O.block_bwd(do, q, k, v, o16, rl, SCALE, False)
    out = (q, k, v, do, o16, np.asarray(rl, np.float32), rdk, rdv)
    for x in out:
        x.setflags(write=False)
    return out


ORACLE_HEADS = [0, 15]


@functools.lru_cache(maxsize=None)
def items_case():
    """The item-switch shape; reference dk, dv for batch 0 and ORACLE_HEADS only."""
    dt, B, S, H = "bfloat16", 2, 2304, 16
    q, k, v, do = _inputs(dt, B, S, S, H, H, 23)
    dev = torch.device("cuda:0")
    tq, tk, tv = (torch.from_numpy(x).to(dev) for x in (q, k, v))
    keep = torch.ones(S, S, dtype=torch.bool, device=dev).tril()
    o = torch.empty((B, S, H, D), dtype=torch.float32, device=dev)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    for b in range(B):                                    # float32 forward of every head (a torch composition, none of the kernels)
        s = torch.einsum("shd,thd->hst", tq[b], tk[b]) * SCALE
        s.masked_fill_(~keep, float("-inf"))
        lse[b] = torch.logsumexp(s, dim=-1)
        o[b] = torch.einsum("hst,thd->shd", torch.exp(s - lse[b][:, :, None]), tv[b])
    o16 = round_to(o.cpu().numpy(), dt)
    lse = lse.cpu().numpy()
    sl = lambda x: np.ascontiguousarray(x[0:1][:, :, ORACLE_HEADS])
    ro, rl = O.attention_ref(sl(q), sl(k), sl(v), True, SCALE)
    o16[0][:, ORACLE_HEADS] = round_to(ro.astype(np.float32), dt)[0]       # the launch and the oracle take the same out and lse
    lse[0][ORACLE_HEADS] = np.asarray(rl, np.float32)[0]
    _, rdk, rdv = O.block_bwd(sl(do), sl(q), sl(k), sl(v), sl(o16), np.ascontiguousarray(lse[0:1][:, ORACLE_HEADS]), SCALE, True)
    out = (q, k, v, do, o16, lse, rdk, rdv)
    for x in out:
        x.setflags(write=False)
    return out


def run(c, dt, causal, keys, heads):
    """(dk, dv) float32 numpy of the forced dK/dV launch (16-bit outputs)."""
    from yunchang_amd import _C
    dev = torch.device("cuda:0")
    td = getattr(torch, dt)
    q, k, v, do, o16 = (torch.from_numpy(np.array(x, dtype=np.float32, order="C")).to(td).to(dev) for x in c[:5])
    lse = torch.from_numpy(np.array(c[5], dtype=np.float32, order="C")).to(dev)
    B, Sq, HQ, _ = q.shape
    delta = torch.empty((B, HQ, Sq), dtype=torch.float32, device=dev)
    _C.bwd_delta(do, o16, delta)
    dk = torch.full(k.shape, float("nan"), dtype=td, device=dev)
    dv = torch.full(k.shape, float("nan"), dtype=td, device=dev)
    _C.flash_bwd(do, q, k, v, lse, delta, None, None, None, SCALE, causal, dk16=dk, dv16=dv,
                 family="row64", only="dkdv", dkdv_keys=keys, dkdv_heads=heads)
    kinds = _C.last_launch_kinds()
    assert "dkdv_row64" in kinds and "dkdv_wave8" not in kinds, kinds
    assert _C.last_dkdv_item_keys() == keys, (_C.last_dkdv_item_keys(), keys)
    return dk.float().cpu().numpy(), dv.float().cpu().numpy()


def _check_ring(dt, Sq, heads):
    c = ring_case(dt, Sq)
    what = f"dkdv256 ring Sq={Sq} heads={heads} {dt}"
    dk, dv = run(c, dt, False, 256, heads)
    dk1, dv1 = run(c, dt, False, 128, heads)
    assert np.array_equal(dk, dk1), what + ": dk differs from the 128-key kernel's"
    assert np.array_equal(dv, dv1), what + ": dv differs from the 128-key kernel's"
    assert_close(dk, c[6], *grad_tol(dt, 4), what + " dk")
    assert_close(dv, c[7], *grad_tol(dt, 4), what + " dv")


@pytest.mark.parametrize("heads", [1, 2, 4])
@pytest.mark.parametrize("Sq", [64, 128, 192, 256, 320, 384, 448])
def test_ring_position_at_every_head_switch(dev, Sq, heads):
    _check_ring("bfloat16", Sq, heads)


def test_ring_position_fp16(dev):
    _check_ring("float16", 320, 2)


def test_item_after_item_in_one_workgroup(dev):
    c = items_case()
    n_items = 2 * 16 * (2304 // 256)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_items == 288 and n_items > cus, (n_items, cus)           # some workgroup runs more than one item
    dk, dv = run(c, "bfloat16", True, 256, 1)
    dk1, dv1 = run(c, "bfloat16", True, 128, 1)
    assert np.array_equal(dk, dk1), "items: dk differs from the 128-key kernel's"
    assert np.array_equal(dv, dv1), "items: dv differs from the 128-key kernel's"
    assert_close(dk[0:1][:, :, ORACLE_HEADS], c[6], *grad_tol("bfloat16", 1), "items dk (batch 0, heads 0 and 15)")
    assert_close(dv[0:1][:, :, ORACLE_HEADS], c[7], *grad_tol("bfloat16", 1), "items dv (batch 0, heads 0 and 15)")
