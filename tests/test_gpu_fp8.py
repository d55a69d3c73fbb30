"""The e4m3 forward (csrc/usp_flash_fwd_fp8.hip) and quantize_fp8 on the GPU, against fp64 attention on the dequantized operands
and the bound derived in tests/fp8_ref.py.  An item is 256 query rows (4 waves x 64), a tile 64 keys."""
import pytest
import torch

import fp8_ref as R

pytestmark = pytest.mark.gpu
D = 128
SCALE = D ** -0.5
dev = torch.device("cuda:0")


def _inputs(B, Sq, Sk, Hq, Hkv, seed):
    """Seeded N(0, 1) quantized on the CPU, every head at a scale of its own: a descale read for the wrong head shows."""
    gen = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, s, h, D, generator=gen) for s, h in ((Sq, Hq), (Sk, Hkv), (Sk, Hkv)))
    return (*R.quantize_cpu(q, [1.0 + 0.5 * h for h in range(Hq)]), *R.quantize_cpu(k, [2.0 - 0.25 * h for h in range(Hkv)]),
            *R.quantize_cpu(v, [0.5 + h for h in range(Hkv)]))


SHAPES = [(1, 1, 1, 1, 1, True), (2, 77, 77, 2, 2, True), (1, 200, 333, 3, 1, True), (1, 333, 200, 2, 2, True),
          (1, 384, 640, 4, 2, False), (1, 130, 1, 2, 1, False),
          (1, 257, 321, 2, 1, True)]            # one-row second item, one-key sixth tile


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,Sq,Sk,Hq,Hkv,causal", SHAPES)
def test_forward_within_the_derived_bound(B, Sq, Sk, Hq, Hkv, causal, out_dtype):
    from yunchang_amd import _C
    from yunchang_amd.kernels import hip_attn_forward
    q8, dq, k8, dk, v8, dv = _inputs(B, Sq, Sk, Hq, Hkv, 7)
    out, lse = hip_attn_forward(q8.to(dev), k8.to(dev), v8.to(dev), causal=causal, q_descale=dq.to(dev), k_descale=dk.to(dev),
                                v_descale=dv.to(dev), out_dtype=out_dtype)
    assert _C.last_launch_kinds() == ("fwd_fp8",) and out.dtype == out_dtype
    R.check(out, lse, *R.attention(q8, k8, v8, dq, dk, dv, SCALE, causal, out_dtype), what=f"{(B, Sq, Sk, Hq, Hkv, causal)}")


def test_operand_order_is_exact_on_planted_needles():
    """Row i's score for key i leads every other by 45 nats or more, so the fp32 row sum IS the needle's term and out must be
    v_descale * v8[needle] bit for bit in bf16 -- for every key of two tiles + 1 (0, the last of a tile, the first of the next, the
    last key among them).  v8 differs from key to key and dim to dim: a key permutation between P^T and V^T, or a wrong lane
    layout of an MFMA operand, puts another value there."""
    from yunchang_amd.kernels import hip_attn_forward
    S, Hq, a = 129, 2, 32.0
    k = torch.zeros(1, S, 1, D)
    k[0, torch.arange(128), 0, torch.arange(128)] = a
    k[0, 128] = -a
    q = k.clone()
    q[0, 128] = 0
    q[0, 128, 0, 0] = -a
    q = q.expand(1, S, Hq, D).contiguous()
    # every finite e4m3 code but +-0 (a sum that starts at +0 cannot return -0) and NaN
    codes = (torch.arange(S)[:, None] * 7 + torch.arange(D)[None, :] * 3) % 126 + 1 + 128 * ((torch.arange(S)[:, None] + torch.arange(D)[None, :]) % 2)
    v8 = codes.to(torch.uint8).view(torch.float8_e4m3fn).reshape(1, S, 1, D)
    dq, dk, dv = torch.tensor([[1.0, 2.0]]), torch.tensor([[0.5]]), torch.tensor([[0.75]])
    q8, k8 = q.to(torch.float8_e4m3fn), k.to(torch.float8_e4m3fn)
    s = torch.einsum("bthd,bshd->bhts", q8.double(), k8.double()) * SCALE * dq.double()[:, :, None, None] * dk.double()
    needle = s.diagonal(dim1=2, dim2=3)
    others = s.masked_fill(torch.eye(S, dtype=torch.bool), float("-inf"))
    assert (torch.exp(others - needle[..., None]).sum(-1) < 2.0 ** -30).all(), "the planted gap does not make the row sum exact"
    out, _ = hip_attn_forward(q8.to(dev), k8.to(dev), v8.to(dev), causal=False, q_descale=dq.to(dev), k_descale=dk.to(dev), v_descale=dv.to(dev))
    want = (v8.float() * 0.75).to(torch.bfloat16).expand(1, S, Hq, D)
    bad = (out.cpu().view(torch.int16) != want.contiguous().view(torch.int16)).any(-1).nonzero()
    assert bad.numel() == 0, f"rows (b, key, head) whose out is not v_descale * v8[needle]: {bad[:8].tolist()}"


def test_running_max_jumps_stay_finite():
    """test_gpu_head_dim_256.py::test_running_max_jumps's input, quantized: one key per 64-key tile is aligned with row 300, so its
    maximum grows tile after tile.  Within the bound and finite everywhere: nothing above 448 reaches the conversion."""
    from yunchang_amd.kernels import hip_attn_forward
    gen = torch.Generator().manual_seed(3)
    q, k, v = torch.randn(1, 512, 1, D, generator=gen), torch.randn(1, 512, 1, D, generator=gen) * 0.1, torch.randn(1, 512, 1, D, generator=gen)
    for t in range(8):
        k[0, 64 * t + 5, 0] = q[0, 300, 0] * (0.5 + 0.25 * t)
    (q8, dq), (k8, dk), (v8, dv) = (R.quantize_cpu(x) for x in (q, k, v))
    out, lse = hip_attn_forward(q8.to(dev), k8.to(dev), v8.to(dev), q_descale=dq.to(dev), k_descale=dk.to(dev), v_descale=dv.to(dev))
    R.check(out, lse, *R.attention(q8, k8, v8, dq, dk, dv, SCALE, False), what="running max")


def _strided(t, dev, pad, poison):
    """`t` as a view with padded row, head and batch strides inside poisoned memory on the device: (view, whole buffer)"""
    B, S, H, W = t.shape
    buf = torch.full((B, S + 1, H + 1, W + pad), poison, dtype=torch.float32).to(t.dtype).to(dev)
    view = buf[:, 1:, :H, :W]
    view.copy_(t.to(dev))
    return view, buf


def test_strided_merged_launch_in_poisoned_memory():
    """_C.flash_fwd on strided views in NaN-filled memory, the keys split in two calls (acc only, then merge_in with every row
    final), against the one-call reference; nothing is written outside the views."""
    from yunchang_amd import _C
    B, Sq, Sk, Hq, Hkv, cut = 1, 200, 333, 3, 1, 192
    q8, dq, k8, dk, v8, dv = _inputs(B, Sq, Sk, Hq, Hkv, 11)
    (tq, _), (tk, _), (tv, _) = (_strided(t, dev, 16, float("nan")) for t in (q8, k8, v8))
    out, obuf = _strided(torch.full((B, Sq, Hq, D), 7.0, dtype=torch.bfloat16), dev, 8, 7.0)
    acc, abuf = _strided(torch.full((B, Sq, Hq, D), 7.0), dev, 4, 7.0)
    lse = torch.full((B, Hq, Sq + 3), 7.0, device=dev)[:, :, :Sq]
    guard = [b.clone() for b in (obuf, abuf)]
    kw = dict(q_descale=dq.to(dev), k_descale=dk.to(dev), v_descale=dv.to(dev))
    _C.flash_fwd(tq, tk[:, :cut], tv[:, :cut], SCALE, True, lse, out=None, acc=acc, final_begin=0, final_end=0, shift=Sk - cut, **kw)
    _C.flash_fwd(tq, tk[:, cut:], tv[:, cut:], SCALE, True, lse, out=out, acc=acc, merge_in=True, shift=0, **kw)
    assert _C.last_launch_kinds() == ("fwd_fp8",)
    R.check(out, lse, *R.attention(q8, k8, v8, dq, dk, dv, SCALE, True), what="strided, merged")
    for buf, view, g in ((obuf, out, guard[0]), (abuf, acc, guard[1])):
        view.fill_(7.0)
        assert torch.equal(buf, g), "a launch wrote outside its view"


def test_more_items_than_cus_and_interleave():
    """4 x 33 x 2 = 264 items of 256 rows on 256 CUs: the second pass of the item walk reuses LDS buffers, accumulators and row
    statistics.  Every element against the reference, and bit for bit against USP_LAUNCH_INTERLEAVE (one workgroup per item)."""
    from yunchang_amd import _C
    B, S, Hq, Hkv = 4, 512, 33, 3
    q8, dq, k8, dk, v8, dv = _inputs(B, S, S, Hq, Hkv, 13)
    got = []
    for interleave in (False, True):
        out = torch.empty(B, S, Hq, D, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(B, Hq, S, device=dev)
        _C.flash_fwd(q8.to(dev), k8.to(dev), v8.to(dev), SCALE, True, lse, out=out, interleave=interleave, q_descale=dq.to(dev),
                     k_descale=dk.to(dev), v_descale=dv.to(dev))
        got.append((out, lse))
    assert torch.equal(got[0][0].view(torch.int16), got[1][0].view(torch.int16)) and torch.equal(got[0][1], got[1][1])
    R.check(*got[0], *R.attention(q8, k8, v8, dq, dk, dv, SCALE, True), what="264 items")


@pytest.mark.parametrize("strided", [False, True])
def test_quantize_fp8(strided):
    from yunchang_amd.kernels import quantize_fp8
    x = torch.randn(2, 300, 3, D, generator=torch.Generator().manual_seed(5)) * torch.tensor([0.3, 1.0, 7.0])[None, None, :, None]
    x[1, :, 1] = 0                                            # an all-zero head: descale 1
    x = x.to(torch.bfloat16)
    xd = _strided(x, dev, 24, float("nan"))[0] if strided else x.to(dev)
    R.check_quantized(x, *quantize_fp8(xd))
    if strided:                                               # ... and the element-wise path: a last stride of 2
        x2 = torch.full((2, 300, 3, 2 * D), float("nan"), dtype=torch.bfloat16, device=dev)[..., ::2]
        x2.copy_(x.to(dev))
        R.check_quantized(x, *quantize_fp8(x2))
