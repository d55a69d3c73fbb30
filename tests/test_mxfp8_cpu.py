"""The MXFP8 forward without a GPU: the feature bit and exports, what usp_flash_fwd_mxfp8 / usp_quantize_mxfp8 decline before anything
is launched (include/usp_hip.h: USP_ATTN_MXFP8), and the rules of kernels/features.py: fp8_alone for block scales."""
import ctypes
import os

import pytest
import torch

from yunchang_amd import _C
from yunchang_amd.kernels import hip_attn_forward, hip_attn_func
from test_fp8_cpu import REFUSED, _args as fp8_args

F8, E8 = torch.float8_e4m3fn, torch.float8_e8m0fnu


def test_feature_bit_exports_and_header():
    L = _C.load()
    assert _C.USP_ATTN_MXFP8 == 4194304 and L.usp_attn_features() & _C.USP_ATTN_MXFP8 and L.usp_abi_version() == 7
    assert _C.MXFP8_EXPORTS == ("usp_flash_fwd_mxfp8", "usp_quantize_mxfp8") and _C.KINDS_MXFP8 == {1048576: "fwd_mxfp8"}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "usp_hip.h")).read()
    for name in _C.MXFP8_EXPORTS:
        assert name in _C.EXPORTS and hasattr(L, name) and f"int {name}(" in header


def _args(D=128):
    a, buf, addr = fp8_args(D)
    a.out, a.final_end = _C.UspTensor(addr, 0, 128 * 4, 128), 16      # (complete: only the case's own fault is left to find)
    return a, buf, addr


DECLINED = [dict(flags=_C.USP_ATTN_SOFTCAP, softcap=30.0), dict(flags=_C.USP_ATTN_WINDOW, window_left=4, window_right=0), dict(seq="packed"),
            dict(flags=_C.USP_FORCE_ROW64), dict(flags=_C.USP_FORCE_WAVE32), dict(D=64), dict(D=256), dict(k_stride_s=136),
            dict(scale_offset=2), dict(scale_stride_s=6)]


@pytest.mark.parametrize("case", DECLINED, ids=lambda c: str(sorted(c.items())))
def test_c_abi_declines_without_a_launch(case):
    L = _C.load()
    fn = _C._feature_entry("usp_flash_fwd_mxfp8")
    a, buf, addr = _args(case.get("D", 128))
    scale = _C.UspTensor(addr + case.get("scale_offset", 0), 0, case.get("scale_stride_s", 16), 4)
    for key, val in case.items():
        if key == "seq":
            a.seq_q = a.seq_k = addr
        elif key == "k_stride_s":                              # rows of one-byte elements off a 16-byte boundary
            a.k = _C.UspTensor(addr, 0, val, 128)
        elif key not in ("D", "scale_offset", "scale_stride_s"):
            setattr(a, key, val)
    s = ctypes.byref(scale)
    assert fn(ctypes.byref(a), s, s, s, 0, None) == -2 and L.usp_last_launch_kinds() == 0
    ok, good = _args()[0], ctypes.byref(_C.UspTensor(addr, 0, 16, 4))
    assert fn(ctypes.byref(ok), good, good, good, 2, None) == -1 and L.usp_last_launch_kinds() == 0          # out_dtype
    assert fn(ctypes.byref(ok), good, None, good, 0, None) == -1 and L.usp_last_launch_kinds() == 0          # all three are required


def test_quantizer_declines():
    fn, t = _C._feature_entry("usp_quantize_mxfp8"), ctypes.byref(_C.UspTensor(4096, 0, 512, 128))
    assert fn(0, 2, t, 1, t, 1, t, 1, 8, 4, 128, None) == -1          # an axis other than the two
    assert fn(0, 0, t, 1, t, 1, None, 1, 8, 4, 128, None) == -1       # no scale
    assert fn(0, 0, t, 1, t, 1, t, 1, 8, 4, 48, None) == -2           # no whole blocks along the head dim


def _q(S=64, H=2, dtype=F8):
    return torch.zeros(1, S, H, 128, dtype=dtype)            # a CPU tensor: any kernel call would raise something else


def _s(S=64, H=2, W=4):
    return torch.full((1, S, H, W), 127, dtype=torch.uint8).view(E8)


GOOD = dict(q_descale=_s(), k_descale=_s(), v_descale=_s(2, 2, 128))


@pytest.mark.parametrize("kw,exc,match", [
    (dict(GOOD, k_descale=torch.ones(1, 2)), NotImplementedError, "k_descale is torch.float32 beside q_descale"),
    (dict(GOOD, v_descale=None), NotImplementedError, "v_descale is None beside q_descale"),
    (dict(GOOD, q_descale=_s(W=2)), ValueError, r"q_descale is \(1, 64, 2, 2\).*\(1, 64, 2, 4\)"),
    (dict(GOOD, v_descale=_s(64, 2, 128)), ValueError, r"v_descale is .*\(1, 2, 2, 128\)"),
    (dict(GOOD, k_descale=_s(W=8)[..., ::2]), ValueError, "k_descale has a last stride of 2"),
    (dict(GOOD, q_descale=_s().to("meta")), ValueError, "q_descale is on meta"),
], ids=["fp32-beside", "none-beside", "q-shape", "v-shape", "k-stride", "device"])
def test_block_scale_rules(kw, exc, match):
    for call in (lambda: hip_attn_forward(_q(), _q(), _q(), **kw), lambda: _C.flash_fwd(_q(), _q(), _q(), 0.1, True, None, **kw)):
        with pytest.raises(exc, match=match):
            call()


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: next(iter(kw)))
def test_every_option_beside_block_scales_is_refused(kw):
    with pytest.raises(NotImplementedError, match=rf"float8_e4m3fn.*{next(iter(kw))}"):
        hip_attn_forward(_q(), _q(), _q(), causal=True, **GOOD, **kw)


def test_good_block_scales_reach_the_kernel_call_and_scales_are_no_operands():
    with pytest.raises(RuntimeError, match="ROCm device tensors"):                  # every rule passed: the launch wants the GPU
        hip_attn_forward(_q(), _q(), _q(), **GOOD)
    with pytest.raises(NotImplementedError, match="forward-only.*hip_attn_forward"):
        hip_attn_func(_s(W=128), _s(W=128), _s(W=128))
    with pytest.raises(NotImplementedError, match="q is torch.float8_e8m0fnu"):
        hip_attn_forward(_s(W=128), _q(), _q())
    with pytest.raises(ValueError, match="mx is 'x'"):
        _C.quantize_fp8(torch.zeros(1, 32, 1, 128, dtype=torch.bfloat16), mx="x")
