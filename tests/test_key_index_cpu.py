"""The gathered-key forward without a GPU: the feature bit and export, what usp_flash_fwd_gather declines before anything is launched
(include/usp_hip.h: USP_ATTN_KEY_INDEX), and the rules of kernels/features.py: key_index_alone."""
import ctypes
import os

import pytest
import torch

from yunchang_amd import _C
from yunchang_amd.kernels import hip_attn_forward
from yunchang_amd.kernels.features import BlockSelect

IDX = torch.zeros(2, 8, dtype=torch.int32)


def _q(D=128, dtype=torch.bfloat16):
    return torch.zeros(1, 64, 2, D, dtype=dtype)             # a CPU tensor: any kernel call would raise something else


def test_feature_bit_export_and_header_line():
    L = _C.load()
    assert _C.USP_ATTN_KEY_INDEX == 8388608 and L.usp_attn_features() & _C.USP_ATTN_KEY_INDEX and L.usp_abi_version() == 7
    assert _C.GATHER_EXPORTS == ("usp_flash_fwd_gather",) and _C.KINDS_GATHER == {2097152: "fwd_gather"}
    assert "usp_flash_fwd_gather" in _C.EXPORTS and hasattr(L, "usp_flash_fwd_gather")
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "usp_hip.h")).read()
    assert "#define USP_ATTN_KEY_INDEX 8388608" in header and "USP_KIND_FWD_GATHER = 2097152" in header
    assert "int usp_flash_fwd_gather(const usp_fwd_args* args, const int32_t* key_index, int64_t index_stride_b," in header


def _args(D=128):
    buf = ctypes.create_string_buffer(1 << 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    a = _C.UspFwdArgs()
    a.dtype, a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D, a.causal, a.softmax_scale = 0, 1, 16, 16, 4, 1, D, 1, 0.0625
    a.q = a.out = _C.UspTensor(addr, 0, D * 4, D)
    a.k = a.v = _C.UspTensor(addr, 0, D, D)
    a.lse, a.final_end = addr, 16
    return a, buf, addr


EINVAL, EUNSUPPORTED = -1, -2
DECLINED = [(dict(idx=None), EINVAL), (dict(n=0), EINVAL), (dict(idx=2), EINVAL),
            (dict(causal=0), EUNSUPPORTED), (dict(D=32), EUNSUPPORTED), (dict(D=256), EUNSUPPORTED),
            (dict(flags=_C.USP_ATTN_WINDOW, window_left=4, window_right=1), EUNSUPPORTED),
            (dict(flags=_C.USP_ATTN_SOFTCAP, softcap=30.0), EUNSUPPORTED), (dict(flags=_C.USP_ATTN_SHIFT, mask_shift=1), EUNSUPPORTED),
            (dict(flags=_C.USP_FORCE_ROW64), EUNSUPPORTED), (dict(flags=_C.USP_FORCE_WAVE32), EUNSUPPORTED), (dict(seq="packed"), EUNSUPPORTED),
            (dict(merge_in=1), EUNSUPPORTED), (dict(acc=True), EUNSUPPORTED), (dict(final_end=8), EUNSUPPORTED)]


@pytest.mark.parametrize("case,rc", DECLINED, ids=lambda c: str(sorted(c.items())) if isinstance(c, dict) else None)
def test_c_abi_declines_without_a_launch(case, rc):
    L = _C.load()
    fn = _C._feature_entry("usp_flash_fwd_gather")
    a, buf, addr = _args(case.get("D", 128))
    idx, n = addr + 64, 8
    for key, val in case.items():
        if key == "idx":
            idx = None if val is None else idx + val           # a NULL list; a list off a 4-byte boundary
        elif key == "n":
            n = val
        elif key == "seq":
            a.seq_q = a.seq_k = addr
        elif key == "acc":
            a.acc = a.out
        elif key != "D":
            setattr(a, key, val)
    assert fn(ctypes.byref(a), idx, 0, 8, n, None) == rc and L.usp_last_launch_kinds() == 0


REFUSED = [dict(softcap=30.0), dict(alibi_slopes=torch.ones(2)), dict(dropout_p=0.1), dict(sinks=torch.zeros(2)), dict(cu_doclens=[0, 32, 64]),
           dict(bidirectional=[(0, 8)]), dict(block_mask=torch.ones(1, 1, dtype=torch.bool)), dict(block_select=BlockSelect(2)),
           dict(return_max_logits=True), dict(return_block_mass=True)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: next(iter(kw)))
def test_every_other_option_is_refused_with_the_usual_sentence(kw):
    name = next(iter(kw))
    with pytest.raises(NotImplementedError, match=rf"key_index together with {name} is not supported by the HIP attention kernels"):
        hip_attn_forward(_q(), _q(), _q(), causal=True, key_index=IDX, **kw)


@pytest.mark.parametrize("q,kw,match", [
    (_q(), dict(window_size=(8, 4)), "key_index together with a window_size whose right bound is not 0 is not supported"),
    (_q(), dict(causal=False), "key_index together with causal=False"), (_q(32), {}, "head_dim 32 together with key_index"),
    (_q(96), {}, "head_dim 96 together with key_index"), (_q(256), {}, "head_dim 256 .*together with key_index"),
    (_q(dtype=torch.float8_e4m3fn), {}, "float8_e4m3fn q, k, v together with key_index"),
], ids=["right", "full", "D32", "D96", "D256", "fp8"])
def test_refusals_by_name(q, kw, match):
    kw = dict(dict(causal=True), **kw)
    for call in (lambda: hip_attn_forward(q, q, q, key_index=IDX, **kw),
                 lambda: _C.flash_fwd(q, q, q, 0.1, kw["causal"], None, window=kw.get("window_size"), key_index=IDX)):
        with pytest.raises(NotImplementedError, match=match):
            call()
    v = _q()
    with pytest.raises(NotImplementedError, match=r"head dims \(192, 128\) of q / k and v together with key_index"):
        hip_attn_forward(_q(192), _q(192), v, causal=True, key_index=IDX)


@pytest.mark.parametrize("idx,match", [(IDX.long(), "int32"), (torch.zeros(3, 8, dtype=torch.int32), "shape"), (IDX[:, ::2], "last stride"),
                                       (torch.zeros(2, 0, dtype=torch.int32), "n >= 1"), (torch.zeros(1, 1, 2, 8, dtype=torch.int32), "shape")],
                         ids=["int64", "heads", "stride", "empty", "4d"])
def test_malformed_lists_are_refused_from_shape_dtype_and_strides(idx, match):
    with pytest.raises(ValueError, match=match):
        hip_attn_forward(_q(), _q(), _q(), causal=True, key_index=idx)


def test_well_formed_cpu_call_reaches_the_device_check_and_none_is_the_old_path():
    for kw in (dict(key_index=IDX), dict(key_index=IDX[0]), dict(key_index=IDX[None]), dict(key_index=IDX, window_size=(8, 0)),
               dict(key_index=None), {}):
        with pytest.raises(RuntimeError, match="ROCm device tensors"):
            hip_attn_forward(_q(), _q(), _q(), causal=True, **kw)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        _C.flash_fwd(_q(), _q(), _q(), 0.1, True, torch.zeros(1, 2, 64), out=_q(), key_index=IDX)
