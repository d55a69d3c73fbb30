"""The antidiagonal block gate (BlockSelectAntidiag, antidiag_block_weights, select_blocks_from_weights) without a GPU: the record's
validation, every refusal sentence, the C entry points declining without a launch, and the fp64 reference pinned to its definition."""
import ctypes

import pytest
import torch

import block_antidiag_ref as AD
import block_mass_ref as MR
from dist_util import run_distributed


def _small():
    q, k = (torch.zeros(1, 256, h, 32, dtype=torch.bfloat16) for h in (4, 2))
    return q, k, k.clone()


def test_record_validation_and_refusals():
    import yunchang_amd as Y
    from yunchang_amd.hybrid.async_attn_layer import AsyncLongContextAttention
    from yunchang_amd.kernels import features as F
    from yunchang_amd.ring.ring_flash_attn_varlen import ring_flash_attn_varlen_func
    from yunchang_amd.ring.zigzag_ring_flash_attn_varlen import zigzag_ring_flash_attn_varlen_func
    sel = Y.BlockSelectAntidiag(0.9)
    assert Y.BlockSelectAntidiag is F.BlockSelectAntidiag and sel == (0.9, 8, 0, 1) and F.block_select_alone(Y.BlockSelectAntidiag(0.9, 16, 1, 2))
    for bad in (0, 1.5, float("nan"), True, "0.5", None):
        with pytest.raises(ValueError, match="top_p must be a real number in \\(0, 1\\]"):
            F.block_select_alone(Y.BlockSelectAntidiag(bad))
    for bad in (0, 1, 2, 3, 32, 8.0, True, None, "8"):
        with pytest.raises(ValueError, match="stride must be one of \\(4, 8, 16\\)"):
            F.block_select_alone(Y.BlockSelectAntidiag(0.9, stride=bad))
    q, k, v = _small()
    with pytest.raises(ValueError, match="keep_local >= 1"):
        Y.select_blocks_antidiag(q, k, 0.9, causal=True, keep_local=0)
    with pytest.raises(NotImplementedError, match="same length"):
        Y.antidiag_block_weights(q, k[:, :128])
    with pytest.raises(NotImplementedError, match="up to 8192 blocks"):                  # (judged before the weights are launched)
        Y.select_blocks_antidiag(q[:, :1].expand(1, 8193 * 128, 4, 32), k[:, :1].expand(1, 8193 * 128, 2, 32), 0.9)
    cu = torch.tensor([0, 256], dtype=torch.int32)
    for fn in (ring_flash_attn_varlen_func, zigzag_ring_flash_attn_varlen_func):
        with pytest.raises(NotImplementedError, match="variable-length.*ring_flash_attn_func"):
            fn(q[0], k[0], v[0], cu, 256, block_select=sel)
    with pytest.raises(NotImplementedError, match="block_select.*AsyncLongContextAttention.*LongContextAttention"):
        AsyncLongContextAttention.forward(None, q, k, v, block_select=sel)


def _ring2_worker(rank, ws):
    import yunchang_amd as Y
    Y.set_seq_parallel_pg(1, 2, rank, ws)
    q, k, v = _small()
    got = []
    for impl in ("basic", "zigzag", "strip"):
        try:
            Y.LongContextAttention(ring_impl_type=impl)(q, k, v, causal=True, block_select=Y.BlockSelectAntidiag(0.9))
            got.append("ran")
        except NotImplementedError as e:
            got.append(str(e))
    return got


def test_ring_degree_2_refuses_on_gloo():
    for got in run_distributed(_ring2_worker, 2):
        assert len(got) == 3 and all("BlockSelectAntidiag at ring degree 2" in m and "use BlockSelectTopP" in m for m in got), got


def test_entry_points_decline_without_launch():
    from yunchang_amd import _C
    wts, sel = _C._feature_entry("usp_block_antidiag_weights"), _C._feature_entry("usp_block_select_weights")
    assert _C.USP_ATTN_BLOCK_SELECT_ANTIDIAG == 2097152 and _C.load().usp_attn_features() & 2097152
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 63) & ~63
    EINVAL, EUNSUP = -1, -2
    ok = dict(dtype=0, B=1, S=256, Hq=4, Hkv=2, D=32, scale=0.1, causal=1, stride=8)

    def weights(q=a, k=a, out=a, qs=(32768, 128, 32), ks=(16384, 64, 32), os_=(16, 4, 2), **kw):
        p = dict(ok, **kw)
        return wts(q, k, p["dtype"], p["B"], p["S"], p["Hq"], p["Hkv"], p["D"], *qs, *ks, p["scale"], p["causal"], p["stride"], out, *os_, None)
    for kw in (dict(q=None), dict(k=None), dict(out=None), dict(B=0), dict(S=0), dict(Hq=0), dict(Hkv=-1), dict(D=0), dict(dtype=2),
               dict(stride=0), dict(stride=2), dict(stride=12), dict(stride=32), dict(qs=(32768, -128, 32)), dict(ks=(-1, 64, 32)),
               dict(os_=(16, 4, -2)), dict(scale=float("nan"))):
        assert weights(**kw) == EINVAL, kw
    for kw in (dict(D=20), dict(D=256), dict(D=96), dict(Hq=3), dict(q=a + 4), dict(k=a + 8), dict(qs=(32768, 132, 32)), dict(ks=(16384, 64, 36)),
               dict(out=a + 1), dict(ks=(16384, 1 << 21, 32)), dict(ks=(16384, 0, 32)), dict(ks=(16384, 24, 32))):     # (k rows that overlap)
        assert weights(**kw) == EUNSUP, kw

    def select(w=a, mask=a, ws=(64, 16, 4), ms=(64, 16, 4), B=1, Hq=4, nbq=4, nbk=4, row0=0, causal=1, top_p=0.9, kf=0, kl=1):
        return sel(w, *ws, B, Hq, nbq, nbk, row0, causal, top_p, kf, kl, mask, *ms, None)
    for kw in (dict(w=None), dict(mask=None), dict(B=0), dict(Hq=0), dict(nbq=0), dict(nbk=-1), dict(row0=-1), dict(kf=-1), dict(kl=-1),
               dict(kl=0), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(ws=(64, -16, 4)), dict(ms=(-64, 16, 4))):
        assert select(**kw) == EINVAL, kw
    assert select(nbk=8193) == EUNSUP and select(w=a + 2) == EUNSUP and _C.load().usp_last_launch_kinds() == 0


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("S,stride,Hq,Hkv", [(128, 4, 2, 2), (257, 8, 2, 1), (300, 16, 4, 2)])
def test_reference_rows_sum_to_one(S, stride, Hq, Hkv, causal):
    g = torch.Generator().manual_seed(S)
    q, k = (torch.randn(1, S, h, 32, generator=g).to(torch.bfloat16) for h in (Hq, Hkv))
    w = AD.weights_ref(q, k, 32 ** -0.5, causal, stride)
    nb = (S + 127) // 128
    assert w.shape == (1, Hq, nb, nb) and torch.allclose(w.sum(-1), torch.ones(1, Hq, nb, dtype=torch.float64), rtol=1e-12, atol=0)
    assert not causal or float(w.triu(1).abs().max()) == 0.0


@pytest.mark.parametrize("stride", [4, 8, 16])
def test_reference_is_the_block_mass_on_patchwise_constant_inputs(stride):
    """q and k constant inside each patch: every (row, key) pair of a patch has the sub-score as its score, so the weights are the
    block attention mass of the same scores (full attention; under causal the patch on the diagonal counts whole, by definition)."""
    g = torch.Generator().manual_seed(stride)
    S, scale = 384, 32 ** -0.5
    q, k = (torch.randn(1, S // stride, h, 32, generator=g).to(torch.bfloat16).repeat_interleave(stride, dim=1) for h in (4, 2))
    s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double().repeat_interleave(2, dim=2)) * scale
    assert torch.allclose(AD.weights_ref(q, k, scale, False, stride), MR.mass_ref(q, k, torch.logsumexp(s, -1), scale, False), rtol=1e-12, atol=1e-300)
