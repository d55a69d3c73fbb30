"""Head dims (192, 128) without a GPU: the one feature rule (kernels/features.py: head_dims_192_128_alone) and what
usp_flash_fwd_vdim / usp_flash_bwd_vdim decline before anything is launched (include/usp_hip.h: USP_ATTN_HEAD_DIMS_192_128)."""
import ctypes

import pytest
import torch

from yunchang_amd import _C
from yunchang_amd.kernels import hip_attn_backward, hip_attn_forward, hip_attn_func
from yunchang_amd.kernels.features import BlockSelect

REFUSED = [dict(window_size=(64, 0)), dict(softcap=30.0), dict(alibi_slopes=torch.ones(2)), dict(dropout_p=0.1), dict(sinks=torch.zeros(2)),
           dict(cu_doclens=[0, 32, 64]), dict(bidirectional=[(0, 8)]), dict(block_mask=torch.ones(1, 1, dtype=torch.bool)),
           dict(block_select=BlockSelect(2)), dict(return_max_logits=True), dict(return_block_mass=True)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: next(iter(kw)))
def test_every_option_is_refused_before_a_tensor_is_read(kw):
    q = torch.zeros(1, 64, 2, 192, dtype=torch.bfloat16)         # CPU tensors: any kernel call would raise something else
    v = torch.zeros(1, 64, 2, 128, dtype=torch.bfloat16)
    name = next(iter(kw))
    for call in (lambda: hip_attn_forward(q, q, v, causal=True, **kw), lambda: hip_attn_func(q, q, v, causal=True, **kw)):
        with pytest.raises(NotImplementedError, match=rf"\(192, 128\).*{name}"):
            call()
    bwd_kw = {k: x for k, x in kw.items() if k not in ("block_select", "return_max_logits", "return_block_mass")}
    if bwd_kw:
        with pytest.raises(NotImplementedError, match=rf"\(192, 128\).*{name}"):
            hip_attn_backward(v, q, q, v, v, torch.zeros(1, 2, 64), q, q, v, bwd_causal=True, **bwd_kw)


@pytest.mark.parametrize("D,Dv", [(192, 64), (128, 64), (128, 192), (256, 128), (160, 128)])
def test_other_unequal_pairs_are_refused_naming_both_dims(D, Dv):
    q = torch.zeros(1, 64, 2, D, dtype=torch.bfloat16)
    v = torch.zeros(1, 64, 2, Dv, dtype=torch.bfloat16)
    for call in (lambda: hip_attn_forward(q, q, v), lambda: hip_attn_func(q, q, v), lambda: _C.flash_fwd(q, q, v, 0.1, True, None),
                 lambda: hip_attn_backward(v, q, q, v, v, torch.zeros(1, 2, 64), q, q, v)):
        with pytest.raises(NotImplementedError, match=f"head_dim {D} of q and k with head_dim {Dv} of v"):
            call()


def _args(cls, D=192):
    buf = ctypes.create_string_buffer(1 << 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    a = cls()
    a.dtype, a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D, a.causal, a.softmax_scale = 0, 1, 16, 16, 4, 1, D, 1, 0.0625
    a.q = _C.UspTensor(addr, 0, 256 * 4, 256)
    a.k = a.v = _C.UspTensor(addr, 0, 256, 256)
    a.lse = addr
    if cls is _C.UspBwdArgs:
        a.dout = a.dq16 = a.q
        a.dk16 = a.dv16 = a.k
        a.delta = addr
    return a, buf, addr


def _entries():
    L = _C.load()
    assert L.usp_attn_features() & _C.USP_ATTN_HEAD_DIMS_192_128 and L.usp_abi_version() == 7
    return ((_C.UspFwdArgs, _C._feature_entry("usp_flash_fwd_vdim")), (_C.UspBwdArgs, _C._feature_entry("usp_flash_bwd_vdim")))


DECLINED = [dict(flags=_C.USP_ATTN_SOFTCAP, softcap=30.0), dict(flags=_C.USP_ATTN_WINDOW, window_left=4, window_right=0),
            dict(seq="packed"), dict(flags=_C.USP_FORCE_ROW64), dict(flags=_C.USP_FORCE_WAVE32), dict(flags=_C.USP_DKDV_KEYS256, bwd_only=True),
            dict(pair=(192, 64)), dict(pair=(128, 64)), dict(pair=(256, 128))]


@pytest.mark.parametrize("case", DECLINED, ids=lambda c: str(sorted(c.items())))
def test_c_abi_declines_without_a_launch(case):
    for cls, fn in _entries():
        if case.get("bwd_only") and cls is _C.UspFwdArgs:
            continue
        D, Dv = case.get("pair", (192, 128))
        a, buf, addr = _args(cls, D)
        for key, val in case.items():
            if key == "seq":
                a.seq_q = a.seq_k = addr
            elif key not in ("bwd_only", "pair"):
                setattr(a, key, val)
        assert fn(ctypes.byref(a), Dv, None) == -2, cls.__name__
        assert _C.load().usp_last_launch_kinds() == 0


def test_c_abi_head_dim_192_alone_has_no_kernels_and_dkdv_heads_is_the_whole_group():
    L = _C.load()
    (fcls, fwd), (bcls, bwd) = _entries()
    a, buf, _ = _args(fcls)
    assert L.usp_flash_fwd(ctypes.byref(a), None) == -2 and fwd(ctypes.byref(a), 192, None) == -2 and fwd(ctypes.byref(a), 0, None) == -1
    for heads in (2, 3):                       # Hq / Hkv = 4: 2 divides it and is still refused, 3 does not
        b, buf, _ = _args(bcls)
        b.dkdv_heads = heads
        assert bwd(ctypes.byref(b), 128, None) == -1 and L.usp_last_launch_kinds() == 0


def test_packed_forms_stripe_varlen_and_the_other_layers_refuse_and_name_the_dense_functions():
    from yunchang_amd import ring as R
    from yunchang_amd.hybrid.async_attn_layer import AsyncLongContextAttention
    q = torch.zeros(1, 64, 2, 192, dtype=torch.bfloat16)
    v = torch.zeros(1, 64, 2, 128, dtype=torch.bfloat16)
    kv128 = torch.zeros(1, 64, 2, 2, 128, dtype=torch.bfloat16)
    t, tv, cu = q[0], v[0], torch.tensor([0, 64], dtype=torch.int32)
    for call in (lambda: R.ring_flash_attn_kvpacked_func(q, kv128), lambda: R.zigzag_ring_flash_attn_kvpacked_func(q, kv128, causal=True),
                 lambda: R.stripe_flash_attn_func(q, q, v, causal=True), lambda: R.ring_flash_attn_varlen_func(t, t, tv, cu, 64),
                 lambda: R.zigzag_ring_flash_attn_varlen_func(t, t, tv, cu, 64, causal=True)):
        with pytest.raises(NotImplementedError, match="ring_flash_attn_func and zigzag_ring_flash_attn_func"):
            call()
    with pytest.raises(NotImplementedError, match="served by LongContextAttention"):
        AsyncLongContextAttention.forward(None, q, q, v, causal=True)
    with pytest.raises(NotImplementedError, match=r"\(192, 128\).*packed"):
        _C.flash_fwd_packed(t, t, tv, cu, cu, 64, 64, 0.07, True, None)
    with pytest.raises(NotImplementedError, match=r"\(192, 128\) together with softcap"):
        _C.flash_bwd(v, q, q, v, None, None, None, None, None, 0.07, True, softcap=30.0)      # judged before any tensor is read


def _attn64(q, k, scale, causal):
    """fp64 scores of one block, bottom-right causal: (B, H, Sq, Sk)"""
    g = q.shape[2] // k.shape[2]
    s = torch.einsum("bthd,bshd->bhts", q.double(), k.double().repeat_interleave(g, dim=2)) * scale
    if causal:
        i, j = torch.arange(q.shape[1])[:, None], torch.arange(k.shape[1])[None, :]
        s = s.masked_fill(j > i + (k.shape[1] - q.shape[1]), float("-inf"))
    return s, g


def _fp64_backend():
    """The fp64 block backend at two widths: tests/oracle_backend.py with fwd and bwd that take a v, out, acc, dout and dv of
    another head dim than q's (the oracle's own assert one width)."""
    from oracle_backend import OracleBlockBackend

    class TwoWidths(OracleBlockBackend):
        def fwd(self, q, k, v, scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None, **kw):
            assert all(x is None for x in kw.values()) and v.shape[:3] == k.shape[:3]
            fe = q.shape[1] if final_end is None else final_end
            s, g = _attn64(q, k, scale, causal)
            l = torch.logsumexp(s, -1)
            p = torch.nan_to_num(torch.exp(s - l[..., None]))
            o = torch.einsum("bhts,bshd->bthd", p, v.double().repeat_interleave(g, dim=2))
            if merge_in:
                new = torch.logaddexp(lse.double(), l)
                w = lambda x: torch.nan_to_num(torch.exp(x - new)).transpose(1, 2)[..., None]
                o, l = acc.double() * w(lse.double()) + o * w(l), new
            lse.copy_(l)
            for dst, a, b in ((out, final_begin, fe), (acc, 0, final_begin), (acc, fe, q.shape[1])):
                if b > a:
                    assert dst.shape[-1] == v.shape[-1]
                    dst[:, a:b].copy_(o[:, a:b])

        def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, scale, causal, accum_dq=False, accum_dk=False, accum_dv=False,
                dq16=None, dk16=None, dv16=None, only=None, **kw):
            assert all(x is None for x in kw.values()) and dout.shape[-1] == v.shape[-1]
            s, g = _attn64(q, k, scale, causal)
            p = torch.nan_to_num(torch.exp(s - lse.double()[..., None]))
            B, Sk, Hkv = k.shape[:3]
            ds = p * (torch.einsum("bthd,bshd->bhts", dout.double(), v.double().repeat_interleave(g, dim=2)) - delta.double()[..., None]) * scale
            vals = dict(dq=torch.einsum("bhts,bshd->bthd", ds, k.double().repeat_interleave(g, dim=2)),
                        dk=torch.einsum("bhts,bthd->bshd", ds, q.double()).reshape(B, Sk, Hkv, g, -1).sum(3),
                        dv=torch.einsum("bhts,bthd->bshd", p, dout.double()).reshape(B, Sk, Hkv, g, -1).sum(3))
            for n, d32, d16, accum in (("dq", dq, dq16, accum_dq), ("dk", dk, dk16, accum_dk), ("dv", dv, dv16, accum_dv)):
                if only in (None, "dq" if n == "dq" else "dkdv"):
                    (d16 if d16 is not None else d32).copy_(vals[n] + d32.double() if accum else vals[n])
    return TwoWidths()


def _gloo_worker(rank, ws, ud, rd, impl):
    """LongContextAttention (and, at ud = 1, the ring function alone) at (192, 128) on gloo, forward and backward, against fp64
    attention on the unsharded tensors: the exchanges, relays and travelling gradients carry two widths."""
    import yunchang_amd as Y
    from yunchang_amd.kernels import set_block_backend
    set_block_backend(_fp64_backend())
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    torch.manual_seed(0)
    S, Hq, Hkv = 64 * ws, 4, 2
    q, k, v, do = (torch.randn(1, S, h, d).to(torch.bfloat16) for h, d in ((Hq, 192), (Hkv, 192), (Hkv, 128), (Hq, 128)))
    ext = Y.EXTRACT_FUNC_DICT[impl]
    loc = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in (q, k, v, do)]
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    s, g = _attn64(qr, kr, 192 ** -0.5, True)
    ref = torch.einsum("bhts,bshd->bthd", torch.softmax(s, -1), vr.repeat_interleave(g, dim=2))
    truth = [ext(t.detach(), rank, world_size=ws, rd=rd, ud=ud) for t in (ref,) + torch.autograd.grad(ref, (qr, kr, vr), do.double())]
    for t in loc[:3]:
        t.requires_grad_(True)
    out = Y.LongContextAttention(ring_impl_type=impl)(*loc[:3], causal=True)
    out.backward(loc[3])
    got = [out.detach(), loc[0].grad, loc[1].grad, loc[2].grad]
    return all(a.shape == t.shape and torch.allclose(a.double(), t, atol=tol, rtol=tol) for a, t, tol in zip(got, truth, (2e-2, 5e-2, 5e-2, 5e-2)))


@pytest.mark.parametrize("ws,ud,rd,impl", [(2, 1, 2, "basic"), (2, 1, 2, "zigzag"), (4, 2, 2, "basic")])
def test_rings_and_the_layer_carry_two_widths_on_gloo(ws, ud, rd, impl):
    from dist_util import run_distributed
    assert all(run_distributed(_gloo_worker, ws, ud, rd, impl))
