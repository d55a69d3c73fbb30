"""Dropout (dropout_p) without a GPU: the generator against the Random123 known answers and against csrc/usp_dropout_rng.h
(compiled here with gcc), the statistics of the mask, the fp64 reference against torch autograd of the written-out formula and
against mutants of itself (the power of the GPU comparison, shown without a GPU), what the C ABI refuses before any launch, the
Python refusals and the seed rule, and the schedules -- the basic ring's (row0, key0) of every launch, the layers' head0, the
global window beside it -- on gloo ranks with a numpy block backend, against the unsharded fp64 reference under the same seed."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import dropout_ref
from dist_util import run_distributed
from golden_util import TOL, assert_close, close_mask, grad_tol
from oracle_backend import OracleBlockBackend, _np, _operand, _put

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "long-context-attention_amd", "csrc")

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
THRESHOLDS = {0.0: 256, 1.0 / 1024: 256, 0.1: 230, 0.5: 128, 0.9: 26, 0.999: 1}

SHIM = r"""
#define USP_DROPOUT_FN
#include "usp_dropout_rng.h"
void shim_philox(const uint32_t* ctr, uint32_t k0, uint32_t k1, uint32_t* out) { usp_philox4x32_10(ctr, k0, k1, out); }
/* keep bytes of a rows x keys window at (row0, key0), one usp_dropout_patch call per element's patch */
void shim_window(uint64_t seed, uint32_t b, uint32_t h, uint32_t row0, uint32_t key0, int rows, int keys, uint8_t* out) {
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < keys; ++j) {
      uint32_t w[4];
      const uint32_t gi = row0 + (uint32_t)i, gj = key0 + (uint32_t)j;
      usp_dropout_patch(seed, b, h, gi >> 2, gj >> 2, w);
      out[i * keys + j] = (uint8_t)((w[gi & 3] >> (8 * (gj & 3))) & 0xff);
    }
}
int shim_keep(uint32_t word, int key_in_patch, uint32_t t) { return usp_dropout_keep(word, key_in_patch, t); }
"""


# ---- 1. known answers, and the header against the Python generator ---------------------------------------------------------------
@pytest.fixture(scope="module")
def header_lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dropout_rng")
    src = tmp / "shim.c"
    src.write_text(SHIM)
    lib = tmp / "libshim.so"
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(lib), "-lm"])
    L = ctypes.CDLL(str(lib))
    L.usp_dropout_threshold.argtypes, L.usp_dropout_threshold.restype = [ctypes.c_float], ctypes.c_int
    L.shim_philox.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    L.shim_window.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                              ctypes.c_int, ctypes.c_void_p]
    L.shim_keep.argtypes, L.shim_keep.restype = [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32], ctypes.c_int
    return L


def test_known_answers_and_header_agreement(header_lib):
    for ctr, key, want in KNOWN:
        got = tuple(int(x) for x in dropout_ref.philox4x32_10(*ctr, *key))
        assert got == want, [hex(x) for x in got]
        c, o = (ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 4)()
        header_lib.shim_philox(c, key[0], key[1], o)
        assert tuple(o) == want, [hex(x) for x in o]
    for p, t in THRESHOLDS.items():
        assert dropout_ref.threshold(p) == t == header_lib.usp_dropout_threshold(p), p
    assert [header_lib.shim_keep(0x80ff0100, j, 128) for j in range(4)] == [1, 1, 0, 0]
    # the mask, byte for byte: three windows x two heads x two batches x two seeds (one above 2^32)
    for seed in (1234, (1 << 40) + 99):
        for row0, key0 in ((0, 0), (4, 8), ((1 << 20) + 4, 1 << 30)):
            want = dropout_ref.keep_bytes(seed, 2, 2, 64, 64, row0, key0, head0=5)
            for b in range(2):
                for h in range(2):
                    got = np.zeros((64, 64), dtype=np.uint8)
                    header_lib.shim_window(seed, b, 5 + h, row0, key0, 64, 64, got.ctypes.data)
                    assert np.array_equal(got, want[b, h]), (seed, row0, key0, b, h)
    # an unaligned window of the reference is the aligned one, cut
    full = dropout_ref.keep_bytes(7, 1, 1, 24, 24)
    assert np.array_equal(dropout_ref.keep_bytes(7, 1, 1, 9, 11, 6, 3), full[:, :, 6:15, 3:14])


# ---- 2. statistics of the mask ----------------------------------------------------------------------------------------------------
def _ncorr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_statistics(header_lib, p):
    S, H, seed = 512, 4, 1234
    assert header_lib.usp_dropout_threshold(p) == dropout_ref.threshold(p)      # the statistics are those of the library's t
    m = dropout_ref.keep_mask(p, seed, 1, H + 1, S, S)[0]              # heads 0..4: 4 pairs (h, h + 1)
    m2 = dropout_ref.keep_mask(p, seed + 1, 1, H, S, S)[0]
    q = dropout_ref.threshold(p) / 256.0
    n = H * S * S
    frac = m[:H].mean()
    sigma = math.sqrt(q * (1 - q) / n)
    print(f"[dropout-stat] p {p}: keep fraction {frac:.5f} against {q:.5f} ({abs(frac - q) / sigma:.2f} sigma)")
    assert abs(frac - q) <= 5 * sigma
    pairs = {"rows": (m[:H, :-1], m[:H, 1:]), "keys": (m[:H, :, :-1], m[:H, :, 1:]), "heads": (m[:H], m[1:H + 1]),
             "seeds": (m[:H], m2)}
    for name, (a, b) in pairs.items():
        c = _ncorr(a, b)
        print(f"[dropout-stat] p {p}: lag-1 correlation along {name} {c:+.2e} ({abs(c) * math.sqrt(a.size):.2f} / sqrt(N))")
        assert abs(c) <= 5 / math.sqrt(a.size), (name, c)
    # the cases measured when the function was chosen (seed 1234, head 5, batch 0): at most 1.4 sigma (1.37 and 0.63)
    one = dropout_ref.keep_mask(p, 1234, 1, 1, S, S, head0=5)
    assert abs(one.mean() - q) <= 1.4 * math.sqrt(q * (1 - q) / one.size)
    assert one.mean() == pytest.approx({0.1: 0.89763, 0.5: 0.50062}[p], abs=5e-6)


# ---- 3. the reference against autograd of the written-out formula, and against mutants of itself -------------------------------------
@pytest.mark.parametrize("Sq,Sk,causal,window,shift", [(24, 40, False, None, 0), (40, 24, True, None, 16), (32, 32, False, (9, 4), 0),
                                                       (24, 40, True, (12, 0), 7), (32, 32, True, None, 0)])
def test_reference_against_autograd(header_lib, Sq, Sk, causal, window, shift):
    B, Hq, Hkv, D, p, seed, at = 2, 4, 2, 16, 0.5, (1 << 33) + 5, (8, 12, 3)
    assert 256.0 / header_lib.usp_dropout_threshold(p) == dropout_ref.rescale(p) == 2.0       # the factor written out below
    g = torch.Generator().manual_seed(3)
    q, k, v, do = (torch.randn(B, s, h, D, generator=g, dtype=torch.float64) for s, h in ((Sq, Hq), (Sk, Hkv), (Sk, Hkv), (Sq, Hq)))
    scale = 0.3
    out, lse, dq, dk, dv = dropout_ref.ref_bwd(do, q, k, v, scale, p, seed, at, causal, window, shift)
    keep = torch.from_numpy(dropout_ref.keep_mask(p, seed, B, Hq, Sq, Sk, *at)).double()       # a constant to autograd
    assert 0.3 < float(keep.mean()) < 0.7
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    i = torch.arange(Sq)[:, None] + (Sk - Sq + shift)
    j = torch.arange(Sk)[None, :]
    left, right = (-1, -1) if window is None else window
    right = 0 if causal else right
    vis = torch.ones(Sq, Sk, dtype=torch.bool)
    if right >= 0:
        vis &= j <= i + right
    if left >= 0:
        vis &= j >= i - left
    assert bool(vis.any(1).all()), "the cases keep every row alive (softmax of an empty row is NaN in the plain formula)"
    outs, lses = [], []
    for b in range(B):
        per_head = []
        for h in range(Hq):
            s = (scale * ql[b, :, h] @ kl[b, :, h // (Hq // Hkv)].T).masked_fill(~vis, float("-inf"))
            per_head.append(2.0 * (torch.softmax(s, -1) * keep[b, h]) @ vl[b, :, h // (Hq // Hkv)])      # 256 / t = 2
            lses.append(torch.logsumexp(s, -1))
        outs.append(torch.stack(per_head, 1))
    o2 = torch.stack(outs)
    o2.backward(do)
    assert torch.allclose(out, o2.detach(), atol=1e-12, rtol=1e-10)
    assert torch.allclose(lse.reshape(-1, Sq), torch.stack(lses).detach(), atol=1e-12, rtol=1e-10)
    for got, want in ((dq, ql.grad), (dk, kl.grad), (dv, vl.grad)):
        assert torch.allclose(got, want, atol=1e-11, rtol=1e-9)
    # p = 0 is the plain function (tests/shift_ref.py)
    import shift_ref
    o0, l0 = dropout_ref.ref_fwd(q, k, v, scale, 0.0, seed, at, causal, window, shift)
    o1, l1 = shift_ref.ref_fwd(q, k, v, scale, causal, window, shift)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)


@pytest.mark.parametrize("causal", [False, True])
def test_mutant_references_are_far_away(header_lib, causal):
    """p = 0.5, S = 128, B2 H4/2 D64, N(0,1) inputs rounded to bf16.  Each wrong reference misses the GPU test's bf16 tolerance
    (atol 2e-2 x 256/t = 4e-2, rtol 2e-2 on out) in at least one element of more than half of the (batch, head, query row)
    rows of `out`, and the gradients' (5e-2 x 2, 5e-2) in more than half of the rows of dq: another seed, head, batch, row or
    key, the word / byte roles of a patch swapped, and a rescale by the factor of a wrong threshold (256 and 64 for 128)."""
    B, Hq, Hkv, D, S, p, seed = 2, 4, 2, 64, 128, 0.5, 1234
    g = torch.Generator().manual_seed(1)
    q, k, v, do = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16) for h in (Hq, Hkv, Hkv, Hq))
    scale = D ** -0.5
    true = dropout_ref.ref_bwd(do, q, k, v, scale, p, seed, (0, 0, 0), causal, out_dtype=q.dtype)
    rs = dropout_ref.rescale(p)
    assert rs == 2.0 == 256.0 / header_lib.usp_dropout_threshold(p)

    def mask(seed=seed, B=B, row0=0, key0=0, head0=0):
        return dropout_ref.keep_mask(p, seed, B, Hq, S, S, row0, key0, head0)
    by = dropout_ref.keep_bytes(seed, B, Hq, S, S)
    swapped = by.reshape(B, Hq, S // 4, 4, S // 4, 4).swapaxes(3, 5).reshape(B, Hq, S, S) < 128
    mutants = {"seed + 1": (mask(seed=seed + 1), rs), "head + 1": (mask(head0=1), rs), "batch + 1": (mask(B=B + 1)[1:], rs),
               "row + 1": (mask(row0=1), rs), "key + 1": (mask(key0=1), rs), "word / byte swapped": (swapped, rs),
               "rescale of t = 256": (mask(), 1.0), "rescale of t = 64": (mask(), 4.0)}
    for name, (m, factor) in mutants.items():
        wrong = dropout_ref.ref_bwd(do, q, k, v, scale, p, seed, (0, 0, 0), causal, out_dtype=q.dtype,
                                    keep=(torch.from_numpy(np.ascontiguousarray(m)).double(), factor))
        fracs = {}
        for idx, what, (atol, rtol) in ((0, "out", TOL["bfloat16"]["out"]), (2, "dq", grad_tol("bfloat16"))):
            ok, _ = close_mask(wrong[idx], true[idx], atol * rs, rtol)
            fracs[what] = float((~torch.as_tensor(ok)).any(-1).double().mean())          # rows (b, i, h) with a miss
        print(f"[dropout-mutant] causal {causal} {name}: rows outside the tolerance: " + " ".join(f"{w} {f:.2f}" for w, f in fracs.items()))
        assert all(f > 0.5 for f in fracs.values()), (name, fracs)


# ---- 4. the C ABI at the host: what is refused before any launch ------------------------------------------------------------------
def _lib():
    from yunchang_amd import _C
    if not os.path.exists(_C.lib_path()):
        pytest.fail("libusp_hip.so is not built: run __graft_entry__.build() first")
    return _C, _C.load()


def _args(_C, cls, addr):
    a = cls()
    a.dtype, a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D = 0, 1, 16, 16, 2, 2, 128
    a.softmax_scale = 0.125
    a.lse = addr
    if cls is _C.UspBwdArgs:
        a.delta = addr
        a.dout.ptr = addr
    a.q.ptr = a.k.ptr = a.v.ptr = addr
    outs = (a.dq, a.dk, a.dv) if cls is _C.UspBwdArgs else (a.out,)
    if cls is _C.UspFwdArgs:
        a.final_end = a.Sq
    for t in outs:
        t.ptr = addr
    for t in (a.q, a.k, a.v) + outs + ((a.dout,) if cls is _C.UspBwdArgs else ()):
        t.stride_b, t.stride_s, t.stride_h = 16 * 2 * 128, 2 * 128, 128
    return a


def test_abi_feature_bit_entry_points_and_unchanged_structs():
    _C, L = _lib()
    txt = open(os.path.join(ROOT, "include", "usp_hip.h")).read()
    assert _C.USP_ATTN_DROPOUT == 512 == int(re.search(r"#define USP_ATTN_DROPOUT (\d+)", txt).group(1))
    assert L.usp_attn_features() & _C.USP_ATTN_DROPOUT
    assert L.usp_attn_features() & (_C.USP_ATTN_WINDOW | _C.USP_ATTN_SOFTCAP | _C.USP_ATTN_SHIFT | _C.USP_ATTN_ALIBI) == 2 | 64 | 128 | 256
    assert L.usp_abi_version() == 7 == _C.ABI_VERSION
    for name in ("usp_flash_fwd_dropout", "usp_flash_bwd_dropout"):
        assert name in _C.DROPOUT_EXPORTS and name in _C.EXPORTS and hasattr(L, name)
        fn = _C._dropout_entry(name)
        assert fn.restype is ctypes.c_int
        assert fn.argtypes[1:] == [ctypes.c_float, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
        assert re.search(r"int " + name + r"\(const usp_(fwd|bwd)_args\* args, float p_drop, uint64_t seed, int32_t row0, int32_t key0, "
                         r"int32_t head0,\s+void\* stream\);", txt), name
    # no struct, field or size changed: the sizes are those of ABI v7 before the entry points existed
    assert (ctypes.sizeof(_C.UspFwdArgs), ctypes.sizeof(_C.UspBwdArgs)) == (296, 504)
    for cls in (_C.UspFwdArgs, _C.UspBwdArgs):
        assert cls._fields_[-1] == ("softcap", ctypes.c_float)
    assert len(re.findall(r"typedef struct", txt)) == 3


def test_abi_declines_without_launch():
    """Host memory stands in for the device pointers: every call below must return before anything is launched."""
    _C, L = _lib()
    buf = ctypes.create_string_buffer(1 << 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    seq = (ctypes.c_int32 * 2)(0, 16)
    for cls, name in ((_C.UspFwdArgs, "usp_flash_fwd_dropout"), (_C.UspBwdArgs, "usp_flash_bwd_dropout")):
        call = _C._dropout_entry(name)

        def go(a, p=0.5, seed=7, row0=0, key0=0, head0=0):
            return call(ctypes.byref(a), p, seed, row0, key0, head0, None)
        a = _args(_C, cls, addr)                       # softcap together with dropout
        a.flags, a.softcap = _C.USP_ATTN_SOFTCAP, 30.0
        assert go(a) == -2
        a = _args(_C, cls, addr)                       # a packed batch
        a.seq_q = a.seq_k = ctypes.addressof(seq)
        if cls is _C.UspBwdArgs:
            a.total_k = 16
        assert go(a) == -2
        a = _args(_C, cls, addr)                       # the 64-row family forced
        a.flags = _C.USP_FORCE_ROW64
        assert go(a) == -2
        a = _args(_C, cls, addr)
        for kw in (dict(row0=2), dict(key0=6), dict(row0=1, key0=4), dict(row0=(1 << 31) - 16), dict(key0=(1 << 31) - 16),
                   dict(row0=(1 << 31) - 4)):
            assert go(a, **kw) == -2, kw               # unaligned offsets; row0 + Sq or key0 + Sk reaching 2^31
        for kw in (dict(p=float("nan")), dict(p=-0.25), dict(p=1.0), dict(p=1.5), dict(p=float("inf")), dict(row0=-4), dict(key0=-4),
                   dict(head0=-1)):
            assert go(a, **kw) == -1, kw               # invalid scalars
        a.flags = _C.USP_FORCE_ROW64                   # ... which come before the declines
        assert go(a, p=1.0) == -1 and go(a, head0=-1) == -1 and go(a, row0=-1) == -1
        a = _args(_C, cls, addr)                       # the existing checks still come first
        a.flags, a.softmax_scale = _C.USP_FORCE_ROW64, 0.0
        assert go(a) == -1
        a = _args(_C, cls, addr)
        a.flags = _C.USP_FORCE_ROW64 | _C.USP_FORCE_WAVE32
        assert go(a) == -1
        assert L.usp_last_launch_kinds() == 0


# ---- 5. Python: refusals, validation, the seed rule ------------------------------------------------------------------------------------
class _Rec:
    """A recording block backend: keeps the keywords of every flash call, computes nothing."""
    name = "rec"

    def __init__(self):
        self.calls = []

    def fwd(self, *a, **kw):
        self.calls.append(("fwd", kw))

    def bwd(self, *a, **kw):
        self.calls.append(("bwd", kw))

    def delta(self, *a):
        pass

    def merge(self):
        return "merge"


def test_python_refusals_and_validation(monkeypatch):
    from yunchang_amd import _C
    from yunchang_amd.kernels import attention as KA
    from yunchang_amd.ring import front_end as FE
    from yunchang_amd.ring.ring_flash_attn_varlen import ring_flash_attn_varlen_func
    from yunchang_amd.ring.zigzag_ring_flash_attn_varlen import zigzag_ring_flash_attn_varlen_func
    q = torch.zeros(2, 16, 4, 64, dtype=torch.bfloat16)
    m = torch.ones(4, dtype=torch.float32)
    assert _C.dropout_value(None) is None and _C.dropout_value(0) is None and _C.dropout_value(0.0) is None
    assert _C.dropout_value(0.25) == 0.25
    for bad in (float("nan"), -0.1, 1.0, 1.5, float("inf")):
        with pytest.raises(ValueError):
            _C.dropout_value(bad)
        with pytest.raises(ValueError):
            KA.hip_attn_func(q, q, q, dropout_p=bad)
    assert _C.dropout_args(None) is None and _C.dropout_args((0.0, 1, 2, 3, 4)) is None
    assert _C.dropout_args((0.5, 9, 4, 8, 1)) == (0.5, 9, 4, 8, 1)
    assert [_C.dropout_threshold(p) for p in THRESHOLDS] == list(THRESHOLDS.values())
    assert _C.dropout_args((1.0 / 1024, -1, -4, 1 << 31, -1)) is None      # threshold 256: off, the rest is not looked at (as in C)
    for bad in ((0.5, -1, 0, 0, 0), (0.5, 1 << 64, 0, 0, 0), (0.5, 1, -4, 0, 0), (0.5, 1, 0, 1 << 31, 0), (0.5, 1, 0, 0, -1)):
        with pytest.raises(ValueError):
            _C.dropout_args(bad)
    # dropout with softcap, or with alibi_slopes: no kernel holds two score-level steps
    for other, kw in (("softcap", dict(softcap=30.0)), ("alibi", dict(alibi_slopes=m))):
        for call in (lambda: KA.hip_attn_func(q, q, q, dropout_p=0.1, **kw),
                     lambda: KA.hip_attn_forward(q, q, q, dropout_p=0.1, rng_state=5, **kw),
                     lambda: KA.hip_attn_backward(q, q, q, q, q, None, q, q, q, dropout_p=0.1, rng_state=5, **kw),
                     lambda: KA.get_block_backend(dropout=(0.1, 5, 0), **{("alibi" if "alibi_slopes" in kw else "softcap"): list(kw.values())[0]})):
            with pytest.raises(NotImplementedError, match=other):
                call()
    with pytest.raises(NotImplementedError):
        KA.Features.of(None, None, False, softcap=30.0, alibi_slopes=None, dropout_p=0.1)
    with pytest.raises(NotImplementedError):
        FE._check_hot_path_args(0.1, (-1, -1), 0.0)                # still refuses: dropout is decided beside it
    # the fwd-only / bwd-only contracts return no state: without one they refuse
    with pytest.raises(NotImplementedError, match="rng_state"):
        KA.hip_attn_forward(q, q, q, dropout_p=0.1)
    with pytest.raises(NotImplementedError, match="rng_state"):
        KA.hip_attn_backward(q, q, q, q, q, None, q, q, q, dropout_p=0.1)
    with pytest.raises(ValueError):
        KA.rng_state_of((1, 2, 3))
    assert KA.rng_state_of(9) == (9, 0, 0, 0) and KA.rng_state_of([9, 4, 8, 1]) == (9, 4, 8, 1)
    # the ring forwards refuse a dropout_p that did not come through the front end (no state)
    with pytest.raises(NotImplementedError, match="rng_state"):
        FE.ring_dropout(0.1, None)
    assert FE.ring_dropout(0.0, None) is None and FE.ring_dropout(0.1, (7, 2)) == (0.1, 7, 2)
    # the packed rings say which ring serves it
    t3 = torch.zeros(32, 4, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 32], dtype=torch.int32)
    for f in (ring_flash_attn_varlen_func, zigzag_ring_flash_attn_varlen_func):
        with pytest.raises(NotImplementedError, match="basic"):
            f(t3, t3, t3, cu, 32, dropout_p=0.1, causal=True)
    # the wrapper: dense calls carry (p, seed, row0, key0, head0), `at` is consumed, packed ones refuse
    rec = _Rec()
    prev = KA.set_block_backend(rec)
    try:
        be = KA.get_block_backend(dropout=(0.25, 99, 6))
        be.fwd(1, shift=5, at=(128, 256))
        be.bwd(2)
        assert rec.calls == [("fwd", {"dropout": (0.25, 99, 128, 256, 6), "shift": 5}), ("bwd", {"dropout": (0.25, 99, 0, 0, 6)})]
        assert be.merge() == "merge"
        for packed in (be.fwd_packed, be.bwd_packed):
            with pytest.raises(NotImplementedError, match="packed"):
                packed()
        assert KA.get_block_backend() is rec and KA.get_block_backend(dropout=(0.0, 1, 0)) is rec and KA.get_block_backend(dropout=None) is rec
    finally:
        KA.set_block_backend(prev)

    # a library without the feature bit
    class Old:
        @staticmethod
        def usp_attn_features():
            return _C.USP_ATTN_WINDOW | _C.USP_ATTN_SOFTCAP | _C.USP_ATTN_SHIFT | _C.USP_ATTN_ALIBI
    monkeypatch.setattr(_C, "load", lambda: Old)
    with pytest.raises(NotImplementedError, match="USP_ATTN_DROPOUT"):
        _C._dropout_entry("usp_flash_fwd_dropout")


def test_one_seed_per_call_reused_by_the_backward():
    from yunchang_amd.kernels import attention as KA
    rec = _Rec()
    prev = KA.set_block_backend(rec)
    try:
        def call(D=64, **kw):
            q, k, v = (torch.zeros(1, 16, h, D, dtype=torch.bfloat16, requires_grad=True) for h in (4, 2, 2))
            res = KA.hip_attn_func(q, k, v, dropout_p=0.25, causal=True, **kw)
            out = res[0] if isinstance(res, tuple) else res
            out.backward(torch.zeros_like(out))
            (f, fk), (b, bk) = rec.calls[-2:]
            assert (f, b) == ("fwd", "bwd") and fk["dropout"] == bk["dropout"], rec.calls[-2:]     # backward reuses the forward's
            return res, fk["dropout"]
        torch.manual_seed(11)
        _, d1 = call()
        _, d2 = call()
        torch.manual_seed(11)
        res, d3 = call(D=96, return_attn_probs=True, dropout_head0=6)         # a padded head dim draws once, like any call
        assert d1[0] == 0.25 and d1[2:] == (0, 0, 0) and d3[2:] == (0, 0, 6)
        assert d1[1] == d3[1] != d2[1] and 0 <= d1[1] < 1 << 63                # reproducible under manual_seed, advancing per call
        assert len(res) == 3 and res[2] is None                                # return_attn_probs: no S_dmask
        torch.manual_seed(11)
        assert KA.draw_seed() == d1[1]
        n = len(rec.calls)
        q = torch.zeros(1, 16, 4, 64, dtype=torch.bfloat16)
        state = torch.random.get_rng_state()
        KA.hip_attn_func(q, q, q, causal=True)                                 # no dropout: no draw, no keyword
        assert torch.equal(state, torch.random.get_rng_state()) and rec.calls[n][1].get("dropout") is None
    finally:
        KA.set_block_backend(prev)


# ---- 6. the schedules on gloo ------------------------------------------------------------------------------------------------------
def _np_scores(q, k, scale, causal, window, shift):
    """(B,Hq,Sq,Sk) fp64 numpy: scale q k^T, -inf outside the mask; written on its own."""
    qn, kn = _np(q), _np(k)
    B, Sq, Hq, _ = qn.shape
    Sk = kn.shape[1]
    kn = np.repeat(kn, Hq // kn.shape[2], axis=2)
    rel = np.arange(Sq)[:, None] + (Sk - Sq + (shift or 0)) - np.arange(Sk)[None, :]            # i + off - j
    s = np.einsum("bihd,bjhd->bhij", qn, kn) * scale
    left, right = (-1, -1) if window is None else window
    right = 0 if causal else right
    vis = np.ones((Sq, Sk), dtype=bool)
    if right >= 0:
        vis &= rel >= -right
    if left >= 0:
        vis &= rel <= left
    return np.where(vis[None, None], s, -np.inf)


class DropoutNumpyBackend(OracleBlockBackend):
    """The block seam in numpy fp64 with `dropout`, `shift` and `window`; logs ("fwd" | "bwd", causal, window, shift, dropout,
    merge_in | accum_dq)."""

    def __init__(self):
        super().__init__()
        self.launches = []

    @staticmethod
    def _keep(dropout, B, Hq, Sq, Sk):
        if dropout is None:
            return np.ones((B, Hq, Sq, Sk)), 1.0
        p, seed, row0, key0, head0 = dropout
        return dropout_ref.keep_mask(p, seed, B, Hq, Sq, Sk, row0, key0, head0).astype(np.float64), dropout_ref.rescale(p)

    def fwd(self, q, k, v, softmax_scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None,
            window=None, k_splits=None, shift=None, dropout=None):
        Sq = q.shape[1]
        fe = Sq if final_end is None else final_end
        for t, what in ((q, "q"), (k, "k"), (v, "v"), (acc, "acc")):
            _operand(t, what)
        _operand(out, "out", 8, 8)
        self.launches.append(("fwd", bool(causal), window, shift, dropout, bool(merge_in)))
        s = _np_scores(q, k, softmax_scale, causal, window, shift)
        keep, rs = self._keep(dropout, q.shape[0], q.shape[2], Sq, k.shape[1])
        with np.errstate(invalid="ignore", divide="ignore"):
            mx = s.max(-1)
            safe = np.where(np.isfinite(mx), mx, 0.0)
            e = np.exp(s - safe[..., None])
            bl = np.where(np.isfinite(mx), safe + np.log(e.sum(-1)), -np.inf)                 # (B,H,Sq): un-dropped
            p = np.where(np.isfinite(bl)[..., None], np.exp(s - np.where(np.isfinite(bl), bl, 0.0)[..., None]), 0.0)
            bo = rs * np.einsum("bhij,bjhd->bihd", p * keep, np.repeat(_np(v), q.shape[2] // v.shape[2], axis=2))
            if merge_in:
                old = _np(lse)
                new = np.logaddexp(old, bl)
                fin = np.isfinite(new)
                w_old = np.where(fin, np.exp(old - np.where(fin, new, 0.0)), 0.0)
                w_blk = np.where(fin, np.exp(bl - np.where(fin, new, 0.0)), 0.0)
                bo = _np(acc) * np.swapaxes(w_old, 1, 2)[..., None] + bo * np.swapaxes(w_blk, 1, 2)[..., None]
                bl = new
        _put(lse, bl)
        if fe > final_begin:
            _put(out[:, final_begin:fe], bo[:, final_begin:fe])
        if final_begin > 0:
            _put(acc[:, :final_begin], bo[:, :final_begin])
        if fe < Sq:
            _put(acc[:, fe:], bo[:, fe:])

    def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale, causal, accum_dq=False, accum_dk=False, accum_dv=False,
            dq16=None, dk16=None, dv16=None, window=None, only=None, shift=None, dropout=None):
        assert only is None
        for t, what in ((dout, "dout"), (q, "q"), (k, "k"), (v, "v"), (dq, "dq"), (dk, "dk"), (dv, "dv")):
            _operand(t, what)
        self.launches.append(("bwd", bool(causal), window, shift, dropout, bool(accum_dq)))
        B, Sq, Hq, D = q.shape
        Sk, Hkv = k.shape[1], k.shape[2]
        g = Hq // Hkv
        s = _np_scores(q, k, softmax_scale, causal, window, shift)
        keep, rs = self._keep(dropout, B, Hq, Sq, Sk)
        ln, dl, don, qn = _np(lse), _np(delta), _np(dout), _np(q)
        fin = np.isfinite(ln)
        with np.errstate(invalid="ignore"):
            p = np.where(fin[..., None], np.exp(s - np.where(fin, ln, 0.0)[..., None]), 0.0)
        vv, kk = np.repeat(_np(v), g, axis=2), np.repeat(_np(k), g, axis=2)
        ds = p * (rs * keep * np.einsum("bihd,bjhd->bhij", don, vv) - dl[..., None]) * softmax_scale
        grads = (np.einsum("bhij,bjhd->bihd", ds, kk),
                 np.einsum("bhij,bihd->bjhd", ds, qn).reshape(B, Sk, Hkv, g, D).sum(3),
                 rs * np.einsum("bhij,bihd->bjhd", p * keep, don).reshape(B, Sk, Hkv, g, D).sum(3))
        for val, dst, d16, accum in zip(grads, (dq, dk, dv), (dq16, dk16, dv16), (accum_dq, accum_dk, accum_dv)):
            tot = val + _np(dst) if accum else val
            _put(d16 if d16 is not None else dst, tot)


B, HQ, HKV, D, CH = 2, 4, 2, 32, 48       # CH rows per rank
P_DROP, TORCH_SEED = 0.5, 321
WINDOWED = (True, (70, 0))                # (causal, window) under USP_RING_WINDOW=global
SCALE = D ** -0.5


def _inputs(ws):
    g = torch.Generator().manual_seed(11)
    return [torch.randn(B, CH * ws, h, D, generator=g).to(torch.bfloat16) for h in (HQ, HKV, HKV, HQ)]


def _call_seed():
    """The seed a call draws right behind torch.manual_seed(TORCH_SEED)."""
    from yunchang_amd.kernels.attention import draw_seed
    state = torch.random.get_rng_state()
    torch.manual_seed(TORCH_SEED)
    seed = draw_seed()
    torch.random.set_rng_state(state)
    return seed


_TRUTH = {}


def _truth(ws, causal, window=None):
    key = (ws, causal, window)
    if key not in _TRUTH:
        q, k, v, do = _inputs(ws)
        r = dropout_ref.ref_bwd(do, q, k, v, SCALE, P_DROP, _call_seed(), (0, 0, 0), causal, window, 0, out_dtype=torch.bfloat16)
        _TRUTH[key] = (r[0],) + r[2:]
    return _TRUTH[key]


def _run_layer(layer, loc, **kw):
    lq, lk, lv = (t.detach().clone().requires_grad_(True) for t in loc[:3])
    torch.manual_seed(TORCH_SEED)                      # every rank seeded alike: one mask for the whole grid
    out = layer(lq, lk, lv, dropout_p=P_DROP, **kw)
    out.backward(loc[3])
    return [t.detach().float().numpy() for t in (out, lq.grad, lk.grad, lv.grad)]


def _worker(rank, ws, ud, rd, kind):
    import torch.distributed as dist
    import yunchang_amd as Y
    from yunchang_amd.kernels import set_block_backend
    be = DropoutNumpyBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    loc = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in _inputs(ws)]
    res = {"refused": [], "cases": {}, "launches": {}}
    os.environ.pop("USP_RING_WINDOW", None)
    if kind == "ulysses":                           # UlyssesAttention over the whole world
        res["cases"][True] = _run_layer(Y.UlyssesAttention(dist.group.WORLD), loc, causal=True)
        res["launches"][True] = list(be.launches)
        return res
    attn = Y.LongContextAttention(ring_impl_type="basic")
    if rd > 1:                                      # the zigzag and stripe rings and the async layer refuse and name the basic ring;
        for layer in (Y.LongContextAttention(ring_impl_type="zigzag"), Y.LongContextAttention(ring_impl_type="strip")):
            try:
                layer(*loc[:3], dropout_p=P_DROP, causal=True)
            except NotImplementedError as e:
                res["refused"].append("basic" in str(e))
        try:                                        # a local length that is no multiple of 4 refuses
            attn(*(t[:, :CH - 1].contiguous() for t in loc[:3]), dropout_p=P_DROP, causal=True)
        except NotImplementedError as e:
            res["refused"].append("multiple of 4" in str(e))
    try:
        Y.AsyncLongContextAttention(ring_impl_type="basic")(*loc[:3], dropout_p=P_DROP, causal=True)
    except NotImplementedError as e:
        res["refused"].append("dropout" in str(e))
    for causal in (True, False):
        del be.launches[:]
        res["cases"][causal] = _run_layer(attn, loc, causal=causal)
        res["launches"][causal] = list(be.launches)
    if rd == 4:                                     # together with the global window: the planner's blocks get the same offsets
        os.environ["USP_RING_WINDOW"] = "global"
        del be.launches[:]
        res["cases"]["win"] = _run_layer(attn, loc, causal=WINDOWED[0], window_size=WINDOWED[1])
        res["launches"]["win"] = list(be.launches)
        os.environ.pop("USP_RING_WINDOW", None)
    if rd == 1 and ud == 1:                         # ring degree 1: every dense ring is one block
        for impl in ("basic", "zigzag", "strip"):
            del be.launches[:]
            res["cases"][impl] = _run_layer(Y.LongContextAttention(ring_impl_type=impl), loc, causal=True)
            res["launches"][impl] = list(be.launches)
    return res


def _check(res, ws, ud, rd, name, causal, window=None):
    import yunchang_amd as Y
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    rs = dropout_ref.rescale(P_DROP)
    for rank in range(ws):
        truth = [ext(t, rank, world_size=ws, rd=rd, ud=ud) for t in _truth(ws, causal, window)]
        for got, want, what in zip(res[rank]["cases"][name], truth, ("out", "dq", "dk", "dv")):
            atol, rtol = TOL["bfloat16"]["out"] if what == "out" else grad_tol("bfloat16", HQ // HKV)
            assert_close(got, want, atol * rs, rtol, f"grid {ud}x{rd} rank {rank} {name} {what}")


@pytest.mark.parametrize("ws,ud,rd", [(2, 1, 2), (4, 1, 4), (4, 2, 2), (2, 2, 1), (4, 4, 1)])
def test_dropout_on_the_basic_ring_and_the_layers(ws, ud, rd):
    """(4, 4, 1): a KV-replicated grid (Hkv = 2 < P = 4): the counter holds the QUERY head."""
    res = run_distributed(_worker, ws, ud, rd, "layer")
    seed = _call_seed()
    c = CH * ws // rd
    hq = HQ // ud
    for rank in range(ws):
        assert res[rank]["refused"] == [True] * (4 if rd > 1 else 1), res[rank]["refused"]
    for causal in (True, False):
        _check(res, ws, ud, rd, causal, causal)
        for rank in range(ws):
            r, u = rank // ud, rank % ud            # ring rank (Ulysses groups are consecutive ranks), Ulysses rank
            steps = [s for s in range(rd) if not (causal and s > r)]
            want = [(P_DROP, seed, r * c, ((r - s) % rd) * c, u * hq) for s in steps]
            for tag in ("fwd", "bwd"):
                got = [x for x in res[rank]["launches"][causal] if x[0] == tag]
                assert [x[4] for x in got] == want, (rank, tag, got, want)
                assert [x[1] for x in got] == [causal and s == 0 for s in steps]
                assert all(x[3] is None for x in got) and [x[5] for x in got] == [i > 0 for i in range(len(steps))]
    if rd == 4:
        from yunchang_amd.ring.window_blocks import WindowPlan
        causal, win = WINDOWED
        _check(res, ws, ud, rd, "win", causal, win)
        for rank in range(ws):
            r = rank // ud
            plan = WindowPlan(rd, c, causal, win[0], win[1], r)
            want = [(P_DROP, seed, r * c, ((r - s) % rd) * c, (rank % ud) * hq) for s in plan.steps]
            for tag in ("fwd", "bwd"):
                got = [x for x in res[rank]["launches"]["win"] if x[0] == tag]
                assert [x[4] for x in got] == want, (rank, tag, got, want)
        assert [len(WindowPlan(4, c, True, 70, 0, r).steps) for r in range(4)] == [1, 2, 3, 3]


def test_ulysses_attention_passes_its_heads():
    res = run_distributed(_worker, 2, 2, 1, "ulysses")
    _check(res, 2, 2, 1, True, True)
    seed = _call_seed()
    for rank in range(2):
        assert [x[4] for x in res[rank]["launches"][True]] == [(P_DROP, seed, 0, 0, rank * (HQ // 2))] * 2


def test_ring_degree_one_is_one_block():
    res = run_distributed(_worker, 1, 1, 1, "layer")
    seed = _call_seed()
    for causal in (True, False):
        _check(res, 1, 1, 1, causal, causal)
    for impl in ("basic", "zigzag", "strip"):
        _check(res, 1, 1, 1, impl, True)
        assert [(x[0], x[4]) for x in res[0]["launches"][impl]] == [(t, (P_DROP, seed, 0, 0, 0)) for t in ("fwd", "bwd")]


def _packed_worker(rank, ws, ud, rd):
    """LongContextAttentionQKVPacked against LongContextAttention on the same tensors (equal head counts) under the same seed."""
    import yunchang_amd as Y
    from yunchang_amd.kernels import set_block_backend
    be = DropoutNumpyBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    g = torch.Generator().manual_seed(13)
    qkv = torch.randn(B, CH * ws, 3, HQ, D, generator=g).to(torch.bfloat16)
    do = torch.randn(B, CH * ws, HQ, D, generator=g).to(torch.bfloat16)
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    lqkv, ldo = (ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in (qkv, do))
    a = lqkv.clone().requires_grad_(True)
    torch.manual_seed(TORCH_SEED)
    out = Y.LongContextAttentionQKVPacked(ring_impl_type="basic")(a, dropout_p=P_DROP, causal=True)
    out.backward(ldo)
    packed_launches = list(be.launches)
    del be.launches[:]
    leaves = [lqkv[:, :, i].clone().requires_grad_(True) for i in range(3)]
    torch.manual_seed(TORCH_SEED)
    o2 = Y.LongContextAttention(ring_impl_type="basic")(*leaves, dropout_p=P_DROP, causal=True)
    o2.backward(ldo)
    same = torch.equal(out, o2) and all(torch.equal(a.grad[:, :, i], leaves[i].grad) for i in range(3))
    return same, [x[4] for x in packed_launches], [x[4] for x in be.launches]


def test_the_packed_layer_is_the_plain_layer():
    for same, packed, plain in run_distributed(_packed_worker, 4, 2, 2):
        assert same and packed == plain and all(d is not None and d[0] == P_DROP for d in packed)
