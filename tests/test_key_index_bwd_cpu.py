"""The gathered-key backward without a GPU: the feature bit, exports and launch kinds, what usp_flash_bwd_gather declines before anything
is launched (include/usp_hip.h: USP_ATTN_KEY_INDEX_BWD), and the keyword's rules in hip_attn_backward / hip_attn_func."""
import ctypes
import os

import pytest
import torch

from yunchang_amd import _C
from yunchang_amd.kernels import hip_attn_backward, hip_attn_func

IDX = torch.zeros(2, 8, dtype=torch.int32)
EINVAL, EUNSUPPORTED = -1, -2


def _q(D=128):
    return torch.zeros(1, 64, 2, D, dtype=torch.bfloat16)    # a CPU tensor: any kernel call would raise something else


def _bwd(q, idx=IDX, **kw):
    kw = dict(dict(bwd_causal=True), **kw)
    return hip_attn_backward(q, q, q, q, q, torch.zeros(1, 2, 64), q, q, q, key_index=idx, **kw)


def _func(q, idx=IDX, **kw):
    if "bwd_causal" in kw:
        kw["causal"] = kw.pop("bwd_causal")
    return hip_attn_func(q, q, q, **dict(dict(causal=True), **kw), key_index=idx)


CALLS = pytest.mark.parametrize("call", [_bwd, _func], ids=["backward", "func"])


def test_feature_bit_exports_kinds_and_header_lines():
    L = _C.load()
    assert _C.USP_ATTN_KEY_INDEX_BWD == 16777216 and L.usp_attn_features() & _C.USP_ATTN_KEY_INDEX_BWD and L.usp_abi_version() == 7
    assert _C.GATHER_BWD_EXPORTS == ("usp_flash_bwd_gather_workspace_bytes", "usp_flash_bwd_gather")
    assert _C.KINDS_GATHER_BWD == {4194304: "dq_gather", 8388608: "dkdv_gather"}
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "usp_hip.h")).read()
    for name in _C.GATHER_BWD_EXPORTS:
        assert name in _C.EXPORTS and name in _C._FEATURE_ENTRIES and hasattr(L, name) and f" {name}(const usp_bwd_args* args" in header
    assert "#define USP_ATTN_KEY_INDEX_BWD 16777216" in header
    assert "USP_KIND_DQ_GATHER = 4194304" in header and "USP_KIND_DKDV_GATHER = 8388608" in header


def _args(D=128):
    buf = ctypes.create_string_buffer(1 << 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    a = _C.UspBwdArgs()
    a.dtype, a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D, a.causal, a.softmax_scale = 0, 1, 16, 16, 4, 1, D, 1, 0.0625
    a.dout = a.q = a.dq = _C.UspTensor(addr, 0, D * 4, D)
    a.k = a.v = a.dk = a.dv = _C.UspTensor(addr, 0, D, D)
    a.lse = a.delta = addr
    a.workspace, a.workspace_bytes = addr, 1 << 20             # (a claim: no case gets as far as a launch)
    return a, buf, addr


DECLINED = [(dict(idx=None), EINVAL), (dict(n=0), EINVAL), (dict(idx=2), EINVAL), (dict(workspace_bytes=2 * 4 * 64 * 128 * 4 - 16), EINVAL),
            (dict(workspace=None), EINVAL), (dict(flags=_C.USP_BWD_SKIP_DQ | _C.USP_BWD_SKIP_DKDV), EINVAL), (dict(delta=None), EINVAL),
            (dict(causal=0), EUNSUPPORTED), (dict(D=32), EUNSUPPORTED), (dict(D=256), EUNSUPPORTED),
            (dict(flags=_C.USP_ATTN_WINDOW, window_left=4, window_right=1), EUNSUPPORTED),
            (dict(flags=_C.USP_ATTN_SOFTCAP, softcap=30.0), EUNSUPPORTED), (dict(flags=_C.USP_ATTN_SHIFT, mask_shift=1), EUNSUPPORTED),
            (dict(flags=_C.USP_FORCE_ROW64), EUNSUPPORTED), (dict(flags=_C.USP_FORCE_WAVE32), EUNSUPPORTED), (dict(seq="packed"), EUNSUPPORTED),
            (dict(q="misaligned"), EUNSUPPORTED)]


@pytest.mark.parametrize("case,rc", DECLINED, ids=lambda c: str(sorted(c.items())) if isinstance(c, dict) else None)
def test_c_abi_declines_without_a_launch(case, rc):
    L = _C.load()
    fn = _C._feature_entry("usp_flash_bwd_gather")
    a, buf, addr = _args(case.get("D", 128))
    assert _C._feature_entry("usp_flash_bwd_gather_workspace_bytes")(ctypes.byref(a), 8) == 2 * 4 * 64 * a.D * 4
    idx, n = addr + 64, 8
    for key, val in case.items():
        if key == "idx":
            idx = None if val is None else idx + val           # a NULL list; a list off a 4-byte boundary
        elif key == "n":
            n = val
        elif key == "seq":
            a.seq_q = a.seq_k = addr
        elif key == "q":
            a.q = _C.UspTensor(addr + 2, 0, a.D * 4, a.D)
        elif key != "D":
            setattr(a, key, val)
    assert fn(ctypes.byref(a), idx, 0, 8, n, None) == rc and L.usp_last_launch_kinds() == 0


REFUSED = [dict(softcap=30.0), dict(alibi_slopes=torch.ones(2)), dict(dropout_p=0.1), dict(sinks=torch.zeros(2)), dict(cu_doclens=[0, 32, 64]),
           dict(bidirectional=[(0, 8)]), dict(block_mask=torch.ones(1, 1, dtype=torch.bool))]


@CALLS
@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: next(iter(kw)))
def test_every_other_option_is_refused_with_the_usual_sentence(call, kw):
    with pytest.raises(NotImplementedError, match=rf"key_index together with {next(iter(kw))} is not supported by the HIP attention kernels"):
        call(_q(), **kw)


@CALLS
@pytest.mark.parametrize("q,kw,match", [
    (_q(), dict(window_size=(8, 4)), "key_index together with a window_size whose right bound is not 0 is not supported"),
    (_q(), dict(bwd_causal=False), "key_index together with causal=False"), (_q(32), {}, "head_dim 32 together with key_index"),
    (_q(256), {}, "head_dim 256 .*together with key_index"),
], ids=["right", "full", "D32", "D256"])
def test_refusals_by_name(call, q, kw, match):
    with pytest.raises(NotImplementedError, match=match):
        call(q, **kw)


@CALLS
@pytest.mark.parametrize("idx,match", [(IDX.long(), "int32"), (torch.zeros(3, 8, dtype=torch.int32), "shape"), (IDX[:, ::2], "last stride")],
                         ids=["int64", "heads", "stride"])
def test_malformed_lists_are_refused_from_shape_dtype_and_strides(call, idx, match):
    with pytest.raises(ValueError, match=match):
        call(_q(), idx)


@CALLS
def test_well_formed_cpu_call_reaches_the_device_check(call):
    for kw in (dict(), dict(window_size=(8, 0))):
        with pytest.raises(RuntimeError, match="ROCm device tensors"):
            call(_q(), IDX, **kw)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        _C.flash_bwd(_q(), _q(), _q(), _q(), torch.zeros(1, 2, 64), torch.zeros(1, 2, 64), None, None, None, 0.1, True,
                     dq16=_q(), dk16=_q(), dv16=_q(), key_index=IDX)
