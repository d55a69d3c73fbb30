"""The MXFP8 forward (csrc/usp_flash_fwd_mxfp8.hip) and quantize_fp8(mx=) on the GPU, against fp64 attention on the dequantized
operands (tests/mxfp8_ref.py).  An item is 256 query rows (4 waves x 64), a tile 64 keys = two 32-key scale blocks."""
import pytest
import torch

import fp8_ref as R
import mxfp8_ref as M

pytestmark = pytest.mark.gpu
D = 128
SCALE = D ** -0.5 / 64
dev = torch.device("cuda:0")
F8 = torch.float8_e4m3fn


def _inputs(B, Sq, Sk, Hq, Hkv, seed):
    """Seeded N(0, 1) with every (token, 32-dim block) cell of q and k and every (32-key block, dim) cell of v multiplied by a seeded
    power of two in 2^-6 .. 2^6, then quantized by the rule on the CPU: a scale byte read from a wrong place is an O(1) error."""
    gen = torch.Generator().manual_seed(seed)
    pow2 = lambda *shape: torch.exp2(torch.randint(-6, 7, shape, generator=gen).float())
    q, k, v = (torch.randn(B, s, h, D, generator=gen) for s, h in ((Sq, Hq), (Sk, Hkv), (Sk, Hkv)))
    q, k = (x * pow2(*x.shape[:3], 4).repeat_interleave(32, 3) for x in (q, k))
    v = v * pow2(B, (Sk + 31) // 32, Hkv, D).repeat_interleave(32, 1)[:, :Sk]
    return (*M.quantize_cpu(q, "d"), *M.quantize_cpu(k, "d"), *M.quantize_cpu(v, "s"))


def _forward(ops, causal, out_dtype=torch.bfloat16, scale=SCALE):
    from yunchang_amd import _C
    from yunchang_amd.kernels import hip_attn_forward
    q8, qs, k8, ks, v8, vs = (t.to(dev) for t in ops)
    out, lse = hip_attn_forward(q8, k8, v8, softmax_scale=scale, causal=causal, q_descale=qs, k_descale=ks, v_descale=vs, out_dtype=out_dtype)
    assert _C.last_launch_kinds() == ("fwd_mxfp8",) and out.dtype == out_dtype
    return out, lse


CASES = [(*s, c) for s in [(64, 64, 2, 2), (65, 97, 4, 2), (300, 300, 4, 1), (1, 129, 2, 2)] for c in (True, False)] + [(200, 40, 2, 1, True)]


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Sq,Sk,Hq,Hkv,causal", CASES)
def test_forward_within_the_derived_bound(Sq, Sk, Hq, Hkv, causal, out_dtype):
    ops = _inputs(1, Sq, Sk, Hq, Hkv, 7)
    R.check(*_forward(ops, causal, out_dtype), *M.attention(*ops, SCALE, causal, out_dtype), what=f"{(Sq, Sk, Hq, Hkv, causal)}")


def _needles(S, a=32.0):
    """q, k of tests/test_gpu_fp8.py's needle test: row i's score for key i leads every other by 45 nats or more."""
    k = torch.zeros(1, S, 1, D)
    k[0, torch.arange(128), 0, torch.arange(128)], k[0, 128] = a, -a
    q = k.clone()
    q[0, 128], q[0, 128, 0, 0] = 0, -a
    return q.expand(1, S, 2, D).contiguous().to(F8), k.to(F8)


def test_v_scale_placement_is_exact_on_planted_needles():
    """Every key of two tiles + 1 takes all the mass of its row in turn, so out[i, d] must be v8[i, d] * 2^(v_scale[i // 32, d] - 127)
    bit for bit (an e4m3 value times a power of two is exact in bf16): the transposing read order against P's, and the scale byte
    of every (32-key block, dim)."""
    S = 129
    q8, k8 = _needles(S)
    i, d = torch.arange(S)[:, None], torch.arange(D)[None, :]
    v8 = ((i * 7 + d * 3) % 126 + 1 + 128 * ((i + d) % 2)).to(torch.uint8).view(F8).reshape(1, S, 1, D)       # no +-0, no NaN
    vs = (127 + (7 * torch.arange(5)[:, None] + d) % 17 - 8).to(torch.uint8).reshape(1, 5, 1, D).view(M.E8)
    one = lambda s: torch.full((1, S, s, 4), 127, dtype=torch.uint8).view(M.E8)
    out, _ = _forward((q8, one(2), k8, one(1), v8, vs), False, scale=D ** -0.5)
    want = M.dequantize(v8, vs, "s").to(torch.bfloat16).expand(1, S, 2, D).contiguous()
    bad = (out.cpu().view(torch.int16) != want.view(torch.int16)).any(-1).nonzero()
    assert bad.numel() == 0, f"rows (b, key, head) whose out is not the needle's v: {bad[:8].tolist()}"


def test_q_and_k_scale_placement():
    """q8 and k8 hold a single 1 per 32-dim block and every (token, head, block) has a scale byte of its own, so a score is a sum of
    four powers of two, exact in fp32: a byte taken from another block or row moves it by a factor of 2 or more."""
    S, Hq = 129, 2
    x = torch.zeros(1, S, Hq, D)
    x[..., [3, 40, 77, 126]] = 1.0
    i, h, blk = torch.arange(S)[:, None, None], torch.arange(Hq)[None, :, None], torch.arange(4)[None, None, :]
    qs = (127 + (i * 3 + blk * 5 + h) % 9 - 4).to(torch.uint8)[None].view(M.E8)
    ks = (127 + (i * 7 + blk * 2) % 9 - 4).to(torch.uint8)[None, :, :1].contiguous().view(M.E8)
    v8, vs = M.quantize_cpu(torch.randn(1, S, 1, D, generator=torch.Generator().manual_seed(2)), "s")
    ops = (x.to(F8), qs, x[:, :, :1].to(F8), ks, v8, vs)
    for causal in (False, True):
        R.check(*_forward(ops, causal, scale=2.0 ** -4), *M.attention(*ops, 2.0 ** -4, causal), what=f"q / k scale bytes, causal {causal}")


def _strided(t, fill):
    """`t` as a view with padded row, head and batch strides inside `fill`-ed memory on the device (one-byte types: `fill` is the
    byte): (view, whole buffer)"""
    B, S, H, W = t.shape
    buf = torch.full((B, S + 1, H + 1, W + (16 if t.dtype == F8 else 4)), fill, dtype=torch.uint8 if t.element_size() == 1 else t.dtype, device=dev)
    view = buf[:, 1:, :H, :W]
    view.copy_(t.to(dev).view(buf.dtype))
    return view.view(t.dtype), buf


def test_strided_merged_launch_in_poisoned_memory():
    """_C.flash_fwd on strided views (scale tensors too) in NaN-filled memory, the keys split in two calls at a block boundary (acc
    only, then merge_in with every row final) against the one-call reference; nothing is written outside the views.  The second
    call's key blocks count from ITS first key."""
    from yunchang_amd import _C
    Sq, Sk, Hq, Hkv, cut = 65, 97, 4, 2, 64
    ops = _inputs(1, Sq, Sk, Hq, Hkv, 11)
    tq, tk, tv = (_strided(t, 0x7f)[0] for t in ops[0::2])          # NaN in e4m3 ...
    sq, sk, sv = (_strided(t, 0xff)[0] for t in ops[1::2])          # ... and in e8m0
    out, obuf = _strided(torch.full((1, Sq, Hq, D), 7.0, dtype=torch.bfloat16), 7.0)
    acc, abuf = _strided(torch.full((1, Sq, Hq, D), 7.0), 7.0)
    lse = torch.full((1, Hq, Sq + 3), 7.0, device=dev)[:, :, :Sq]
    guard = [b.clone() for b in (obuf, abuf)]
    _C.flash_fwd(tq, tk[:, :cut], tv[:, :cut], SCALE, True, lse, out=None, acc=acc, final_begin=0, final_end=0, shift=Sk - cut,
                 q_descale=sq, k_descale=sk[:, :cut], v_descale=sv[:, :cut // 32])
    _C.flash_fwd(tq, tk[:, cut:], tv[:, cut:], SCALE, True, lse, out=out, acc=acc, merge_in=True, shift=0,
                 q_descale=sq, k_descale=sk[:, cut:], v_descale=sv[:, cut // 32:])
    assert _C.last_launch_kinds() == ("fwd_mxfp8",)
    R.check(out, lse, *M.attention(*ops, SCALE, True), what="strided, merged")
    for buf, view, g in ((obuf, out, guard[0]), (abuf, acc, guard[1])):
        view.fill_(7.0)
        assert torch.equal(buf, g), "a launch wrote outside its view"


def test_more_items_than_cus_and_interleave():
    """4 x 33 x 2 = 264 items of 256 rows on 256 CUs: the second pass of the item walk reloads the Q scales and restarts the scale
    prefetch.  Every element against the reference, and bit for bit against USP_LAUNCH_INTERLEAVE (one workgroup per item)."""
    from yunchang_amd import _C
    B, S, Hq, Hkv = 4, 512, 33, 3
    ops = _inputs(B, S, S, Hq, Hkv, 13)
    q8, qs, k8, ks, v8, vs = (t.to(dev) for t in ops)
    got = []
    for interleave in (False, True):
        out = torch.empty(B, S, Hq, D, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(B, Hq, S, device=dev)
        _C.flash_fwd(q8, k8, v8, SCALE, True, lse, out=out, interleave=interleave, q_descale=qs, k_descale=ks, v_descale=vs)
        got.append((out, lse))
    assert torch.equal(got[0][0].view(torch.int16), got[1][0].view(torch.int16)) and torch.equal(got[0][1], got[1][1])
    R.check(*got[0], *M.attention(*ops, SCALE, True), what="264 items")


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("S", [64, 77])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("axis", ["d", "s"])
def test_quantize_mx_bit_for_bit(axis, dtype, S, strided):
    """Bytes and elements against the rule computed with torch on the CPU; an all-zero block, a block whose quotient (480) passes
    448, a ragged row block (S = 77), and with `strided` both the padded-row and the element-wise (last stride 2) paths."""
    from yunchang_amd.kernels import quantize_fp8
    x = torch.randn(2, S, 3, D, generator=torch.Generator().manual_seed(5)) * torch.tensor([2.0 ** -9, 1.0, 300.0])[None, None, :, None]
    x[0, :32, 0, :32] = 0
    x[0, 32:64, 1, 32:64] = 0.5
    x[0, 40, 1, 37] = 1.875
    x = x.to(dtype)
    want8, wants = M.quantize_cpu(x, axis)
    views = [x.to(dev)]
    if strided:
        views = [_strided(x, float("nan"))[0], torch.full((2, S, 3, 2 * D), float("nan"), dtype=dtype, device=dev)[..., ::2]]
        views[1].copy_(x.to(dev))
    for xd in views:
        x8, scale = quantize_fp8(xd, mx=axis)
        assert scale.dtype == M.E8 and torch.equal(scale.cpu().view(torch.uint8), wants.view(torch.uint8)), "scale bytes"
        assert torch.equal(x8.cpu().view(torch.uint8), want8.view(torch.uint8)), "elements"
