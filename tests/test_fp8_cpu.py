"""The e4m3 forward without a GPU: the one feature rule (kernels/features.py: fp8_alone), what usp_flash_fwd_fp8 declines before
anything is launched (include/usp_hip.h: USP_ATTN_FP8), and who refuses 8-bit tensors."""
import ctypes

import pytest
import torch

from yunchang_amd import _C
from yunchang_amd.kernels import hip_attn_backward, hip_attn_forward, hip_attn_func
from yunchang_amd.kernels.features import BlockSelect

F8 = torch.float8_e4m3fn
REFUSED = [dict(window_size=(64, 0)), dict(softcap=30.0), dict(alibi_slopes=torch.ones(2)), dict(dropout_p=0.1), dict(sinks=torch.zeros(2)),
           dict(cu_doclens=[0, 32, 64]), dict(bidirectional=[(0, 8)]), dict(block_mask=torch.ones(1, 1, dtype=torch.bool)),
           dict(block_select=BlockSelect(2)), dict(return_max_logits=True), dict(return_block_mass=True)]


def _q(D=128, dtype=F8):
    return torch.zeros(1, 64, 2, D, dtype=dtype)             # a CPU tensor: any kernel call would raise something else


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: next(iter(kw)))
def test_every_option_is_refused_before_a_tensor_is_read(kw):
    with pytest.raises(NotImplementedError, match=rf"float8_e4m3fn.*{next(iter(kw))}"):
        hip_attn_forward(_q(), _q(), _q(), causal=True, **kw)


@pytest.mark.parametrize("q,k,v,kw,match", [
    (_q(64), _q(64), _q(64), {}, "head_dim 64 of q"), (_q(256), _q(256), _q(256), {}, "head_dim 256 of q"),
    (_q(), _q(dtype=torch.bfloat16), _q(), {}, "mixed dtypes"), (_q(dtype=torch.bfloat16), _q(dtype=torch.bfloat16), _q(), {}, "mixed dtypes"),
    (_q(dtype=torch.bfloat16),) * 3 + (dict(k_descale=torch.ones(1, 2)), "k_descale goes with torch.float8_e4m3fn"),
    (_q(dtype=torch.float8_e4m3fnuz),) * 3 + ({}, "q is torch.float8_e4m3fnuz"), (_q(), _q(), _q(dtype=torch.float8_e5m2), {}, "v is torch.float8_e5m2"),
], ids=["D64", "D256", "k16", "v8", "descale16", "fnuz", "e5m2"])
def test_other_dims_and_dtypes_are_refused_by_name(q, k, v, kw, match):
    for call in (lambda: hip_attn_forward(q, k, v, **kw), lambda: _C.flash_fwd(q, k, v, 0.1, True, None, **kw)):
        with pytest.raises(NotImplementedError, match=match):
            call()


def test_everything_else_names_hip_attn_forward():
    from yunchang_amd import ring as R
    from yunchang_amd.hybrid.async_attn_layer import AsyncLongContextAttention
    from yunchang_amd.hybrid.attn_layer import LongContextAttention, LongContextAttentionQKVPacked
    from yunchang_amd.ulysses.attn_layer import UlyssesAttention
    q, t, cu = _q(), _q()[0], torch.tensor([0, 64], dtype=torch.int32)
    kv, qkv = torch.zeros(1, 64, 2, 2, 128, dtype=F8), torch.zeros(1, 64, 3, 2, 128, dtype=F8)
    calls = [lambda: hip_attn_func(q, q, q), lambda: hip_attn_backward(q, q, q, q, q, torch.zeros(1, 2, 64), q, q, q),
             lambda: R.ring_flash_attn_func(q, q, q), lambda: R.zigzag_ring_flash_attn_func(q, q, q, causal=True),
             lambda: R.stripe_flash_attn_func(q, q, q, causal=True), lambda: R.ring_flash_attn_kvpacked_func(q, kv),
             lambda: R.zigzag_ring_flash_attn_qkvpacked_func(qkv, causal=True), lambda: R.ring_flash_attn_varlen_func(t, t, t, cu, 64),
             lambda: R.zigzag_ring_flash_attn_varlen_func(t, t, t, cu, 64, causal=True), lambda: LongContextAttentionQKVPacked.forward(None, qkv)]
    calls += [lambda c=cls: c.forward(None, q, q, q) for cls in (LongContextAttention, AsyncLongContextAttention, UlyssesAttention)]
    for call in calls:
        with pytest.raises(NotImplementedError, match="forward-only.*hip_attn_forward"):
            call()


def _args(D=128):
    buf = ctypes.create_string_buffer(1 << 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    a = _C.UspFwdArgs()
    a.dtype, a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D, a.causal, a.softmax_scale = 0, 1, 16, 16, 4, 1, D, 1, 0.0625
    a.q = _C.UspTensor(addr, 0, 128 * 4, 128)
    a.k = a.v = _C.UspTensor(addr, 0, 128, 128)
    a.lse = addr
    return a, buf, addr


DECLINED = [dict(flags=_C.USP_ATTN_SOFTCAP, softcap=30.0), dict(flags=_C.USP_ATTN_WINDOW, window_left=4, window_right=0), dict(seq="packed"),
            dict(flags=_C.USP_FORCE_ROW64), dict(flags=_C.USP_FORCE_WAVE32), dict(D=64), dict(D=256), dict(D=192), dict(k_stride_s=136),
            dict(q_offset=8)]


@pytest.mark.parametrize("case", DECLINED, ids=lambda c: str(sorted(c.items())))
def test_c_abi_declines_without_a_launch(case):
    L = _C.load()
    assert L.usp_attn_features() & _C.USP_ATTN_FP8 and L.usp_abi_version() == 7
    fn = _C._feature_entry("usp_flash_fwd_fp8")
    a, buf, addr = _args(case.get("D", 128))
    for key, val in case.items():
        if key == "seq":
            a.seq_q = a.seq_k = addr
        elif key == "k_stride_s":                              # rows of one-byte elements off a 16-byte boundary
            a.k = _C.UspTensor(addr, 0, val, 128)
        elif key == "q_offset":
            a.q = _C.UspTensor(addr + val, 0, 512, 128)
        elif key != "D":
            setattr(a, key, val)
    assert fn(ctypes.byref(a), None, None, None, 0, None) == -2 and L.usp_last_launch_kinds() == 0
    assert fn(ctypes.byref(_args()[0]), None, None, None, 2, None) == -1 and L.usp_last_launch_kinds() == 0     # out_dtype
