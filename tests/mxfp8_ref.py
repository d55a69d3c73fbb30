"""Reference of the MXFP8 forward (include/usp_hip.h: USP_ATTN_MXFP8) and of quantize_fp8(mx=).

x8.double() * 2^(byte - 127) is exact, so the reference is fp64 attention on the dequantized operands and the bound is that of
tests/fp8_ref.py, term by term on them: the P rounding and the fp32 chains are the per-head kernel's, and the block scales are
exact powers of two applied to exact products."""
import torch

import fp8_ref as R

E8 = torch.float8_e8m0fnu


def quantize_cpu(x, axis):
    """The OCP MX v1.0 rule on the CPU: (x8 e4m3fn, scale e8m0) of a (B, S, H, D) tensor, blocks of 32 along axis "d" or "s"."""
    xf = x.float()
    B, S, H, D = xf.shape
    if axis == "s":
        xf = torch.cat([xf, xf.new_zeros(B, -S % 32, H, D)], 1).transpose(1, 3)          # (B, D, H, S'): blocks along the last dim
    blocks = xf.reshape(*xf.shape[:3], -1, 32)
    amax = blocks.abs().amax(-1, keepdim=True)
    e = (torch.frexp(amax).exponent - 1 - 8).clamp(-127, 127)                             # floor(log2(amax)) - 8
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    x8 = torch.ldexp(blocks, -e).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).reshape(xf.shape)
    scale = (e.squeeze(-1) + 127).to(torch.uint8)
    if axis == "s":
        x8, scale = x8.view(torch.uint8).transpose(1, 3)[:, :S].contiguous().view(torch.float8_e4m3fn), scale.transpose(1, 3).contiguous()
    return x8, scale.view(E8)


def dequantize(x8, scale, axis):
    f = torch.exp2(scale.view(torch.uint8).double() - 127).repeat_interleave(32, dim=3 if axis == "d" else 1)
    return x8.double() * f[:, :x8.shape[1]]


def attention(q8, qs, k8, ks, v8, vs, scale, causal, out_dtype=torch.bfloat16, shift=0):
    """(out, lse, bound) in fp64: fp8_ref.attention on the dequantized operands."""
    q, k, v = dequantize(q8, qs, "d"), dequantize(k8, ks, "d"), dequantize(v8, vs, "s")
    one = lambda t: torch.ones(t.shape[0], t.shape[2], dtype=torch.float64)
    return R.attention(q, k, v, one(q), one(k), one(v), scale, causal, out_dtype, shift)
