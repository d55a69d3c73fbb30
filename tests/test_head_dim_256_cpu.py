"""Head dim 256 without a GPU: the padding map, the one feature rule (kernels/features.py: head_dim_256_alone), and what
usp_flash_fwd / usp_flash_bwd decline at D = 256 before anything is launched (include/usp_hip.h: USP_ATTN_HEAD_DIM_256)."""
import ctypes

import pytest
import torch

from yunchang_amd import _C
from yunchang_amd.kernels import hip_attn_backward, hip_attn_forward, hip_attn_func
from yunchang_amd.kernels.attention import block_attention_mass, kernel_head_dim, select_blocks, select_blocks_top_p
from yunchang_amd.kernels.features import BlockSelect


def test_head_dims_up_to_256_map_to_a_kernel_once_switched_on():
    from yunchang_amd.kernels import set_head_dim_256
    with pytest.raises(NotImplementedError, match="set_head_dim_256"):       # off by default: the refusal callers know
        kernel_head_dim(129)
    prev = set_head_dim_256(True)
    try:
        assert [kernel_head_dim(d) for d in (128, 129, 160, 192, 256)] == [128, 256, 256, 256, 256]
        with pytest.raises(NotImplementedError):
            kernel_head_dim(264)
    finally:
        set_head_dim_256(prev)


REFUSED = [dict(window_size=(64, 0)), dict(softcap=30.0), dict(alibi_slopes=torch.ones(2)), dict(dropout_p=0.1), dict(sinks=torch.zeros(2)),
           dict(cu_doclens=[0, 32, 64]), dict(bidirectional=[(0, 8)]), dict(block_mask=torch.ones(1, 1, dtype=torch.bool)),
           dict(block_select=BlockSelect(2)), dict(return_max_logits=True), dict(return_block_mass=True)]


@pytest.mark.parametrize("D", [192, 256])
@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: next(iter(kw)))
def test_every_option_is_refused_before_a_tensor_is_read(D, kw):
    q = torch.zeros(1, 64, 2, D, dtype=torch.bfloat16)           # a CPU tensor: any kernel call would raise something else
    name = next(iter(kw))
    for call in (lambda: hip_attn_forward(q, q, q, causal=True, **kw), lambda: hip_attn_func(q, q, q, causal=True, **kw)):
        with pytest.raises(NotImplementedError, match=f"head_dim {D} .*{name}"):
            call()
    bwd_kw = {k: v for k, v in kw.items() if k not in ("block_select", "return_max_logits", "return_block_mass")}
    if bwd_kw:
        with pytest.raises(NotImplementedError, match=f"head_dim {D} .*{name}"):
            hip_attn_backward(q, q, q, q, q, torch.zeros(1, 2, 64), q, q, q, bwd_causal=True, **bwd_kw)


def test_stand_alone_calls_and_packed_batches_are_refused_by_the_rule():
    """(Matched on the rule's own wording: the refusal of every head dim above 128 that it replaces reads otherwise.)"""
    from yunchang_amd.ring import zigzag_ring_flash_attn_varlen_func
    q = torch.zeros(1, 128, 2, 256, dtype=torch.bfloat16)
    t = torch.zeros(128, 2, 256, dtype=torch.bfloat16)
    cu = torch.tensor([0, 128], dtype=torch.int32)
    for call in (lambda: select_blocks(q, q, 1), lambda: select_blocks_top_p(q, q, 0.9),
                 lambda: block_attention_mass(q, q, torch.zeros(1, 2, 128)),
                 lambda: _C.flash_fwd_packed(t, t, t, cu, cu, 128, 128, 0.0625, True, None),
                 lambda: zigzag_ring_flash_attn_varlen_func(t, t, t, cu, 128, causal=True)):
        with pytest.raises(NotImplementedError, match=r"kernel head dim 256\) together with"):
            call()


def _args(cls):
    buf = ctypes.create_string_buffer(1 << 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    a = cls()
    a.dtype, a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D, a.causal, a.softmax_scale = 0, 1, 16, 16, 4, 1, 256, 1, 0.0625
    a.q = _C.UspTensor(addr, 0, 256 * 4, 256)
    a.k = a.v = _C.UspTensor(addr, 0, 256, 256)
    a.lse = addr
    return a, buf, addr


DECLINED = [dict(flags=_C.USP_ATTN_SOFTCAP, softcap=30.0), dict(flags=_C.USP_ATTN_WINDOW, window_left=4, window_right=0),
            dict(seq="packed"), dict(flags=_C.USP_FORCE_ROW64), dict(flags=_C.USP_FORCE_WAVE32), dict(flags=_C.USP_DKDV_KEYS256, bwd_only=True)]


@pytest.mark.parametrize("case", DECLINED, ids=lambda c: str(sorted(c.items())))
def test_c_abi_declines_at_head_dim_256_without_a_launch(case):
    L = _C.load()
    assert L.usp_attn_features() & 262144 and L.usp_abi_version() == 7
    for cls, fn in ((_C.UspFwdArgs, L.usp_flash_fwd), (_C.UspBwdArgs, L.usp_flash_bwd)):
        if case.get("bwd_only") and cls is _C.UspFwdArgs:
            continue
        a, buf, addr = _args(cls)
        if cls is _C.UspBwdArgs:
            a.dout = a.dq16 = a.q
            a.dk16 = a.dv16 = a.k
            a.delta = addr
        for key, val in case.items():
            if key == "seq":
                a.seq_q = a.seq_k = addr
            elif key != "bwd_only":
                setattr(a, key, val)
        assert fn(ctypes.byref(a), None) == -2, cls.__name__
        assert L.usp_last_launch_kinds() == 0


@pytest.mark.parametrize("heads", [2, 3])
def test_dkdv_heads_must_be_the_whole_group_at_head_dim_256(heads):
    L = _C.load()
    b, buf, addr = _args(_C.UspBwdArgs)
    b.dout = b.dq16 = b.q
    b.dk16 = b.dv16 = b.k
    b.delta = addr
    b.dkdv_heads = heads                       # Hq / Hkv = 4: 2 divides it and is still refused, 3 does not
    assert L.usp_flash_bwd(ctypes.byref(b), None) == -1
    assert L.usp_last_launch_kinds() == 0
