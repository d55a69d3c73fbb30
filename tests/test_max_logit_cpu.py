"""return_max_logits without a GPU: a fp64 model of the kernel's tile walk whose mutants show that the chosen inputs see each trap
(the lazily raised reference, the still unmasked tile that opens the generic tail, a masked key, a lost tile, an overwriting merge,
the wrong head's row), the refusal matrix, what the C ABI refuses before any launch (usp_flash_fwd_maxlogit / usp_row_max_reduce),
the feature bit, the keyword off leaving the backend calls as they were, and the schedules -- the basic, zigzag and stripe rings at
degree 2 and 4, Ulysses 2, the 2 x 2 grid, the global window beside it -- on gloo ranks with an oracle backend that serves
`row_max=` (tests/max_logit_ref.py), against the single-process value."""
import ctypes
import os
import re

import pytest
import torch

import max_logit_ref as R
import needle_inputs as NI
from dist_util import run_distributed
from shift_ref import visible

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KBN = 64
LOG2E = 1.4426950408889634


# ---- 1. a model of the kernel's walk, and its mutants ---------------------------------------------------------------------------
def model_row_max(q, k, scale, causal, window=None, waves=4, mutant=None, lost=1):
    """csrc/usp_flash_fwd_body.inc with MAXL, restated in fp64 for ONE launch: per 32-row wave of every (32 * waves)-row item the
    tiles no bound cuts take the pipelined loop (the first one in front of it; the loop's last iteration forms the maximum of tile
    n_main UNMASKED and must not fold it), the rest the generic tail behind the mask; the window form walks rotated.  Keys past Sk
    read as zero, as the buffer loads deliver them.  m_run is raised lazily in the pipelined loop (a wave-uniform decision, 8 / c
    above the reference).  -> (B, Hq, Sq) fp64 in score units.
    mutant: "lazy" (m_run reported) | "nmain" (tile n_main folded unmasked) | "nomask" (a masked tile folded unmasked) |
    "lost" (walk index `lost` skipped)."""
    B, Sq, Hq, D = q.shape
    Sk, G = k.shape[1], q.shape[2] // k.shape[2]
    kbm = 32 * waves
    off = Sk - Sq
    left = -1 if window is None else window[0]
    right = 0 if causal else (-1 if window is None else window[1])
    bounded = right >= 0
    coff = off + max(right, 0)
    vis = visible(Sq, Sk, causal, window)
    nt_pad = -(-Sk // KBN) * KBN
    raw = torch.einsum("bihd,bjhd->bhij", q.double(), k.double().repeat_interleave(G, dim=2))
    raw = torch.nn.functional.pad(raw, (0, nt_pad - Sk))                       # keys past Sk: zero rows of K
    vis = torch.nn.functional.pad(vis, (0, nt_pad - Sk))
    masked = raw.masked_fill(~vis, float("-inf"))
    out = torch.full((B, Hq, Sq), float("-inf"), dtype=torch.float64)
    thr = 8.0 / (scale * LOG2E)
    for q0 in range(0, Sq, kbm):
        blk_last = min(q0 + kbm, Sq) - 1
        blk_end = min(Sk, blk_last + coff + 1) if bounded else Sk
        nt = -(-blk_end // KBN) if blk_end > 0 else 0
        for qw in range(q0, min(q0 + kbm, Sq), 32):
            rows = slice(qw, min(qw + 32, Sq))
            n_full = Sk // KBN
            if bounded:
                n_full = min(n_full, max(0, qw + coff + 1) // KBN)
            if qw + 32 > Sq:
                n_full = 0
            n_full = min(n_full, nt)
            rot = 0
            if left >= 0:
                rot = -(-max(0, q0 + kbm - 1 + off - left) // KBN)
                rot, n_full = (0, 0) if rot >= nt else (rot, max(0, n_full - rot))
            walk = [(j + rot) % nt for j in range(nt)]
            tile = lambda src, t: src[:, :, rows, t * KBN:(t + 1) * KBN].amax(-1)
            m_true = torch.full((B, Hq, rows.stop - rows.start), float("-inf"), dtype=torch.float64)
            m_run = m_true.clone()

            def lazily(mt):                      # the rescale: taken by the whole wave when ANY of its rows is 8 / c above
                nonlocal m_run
                if bool((mt > m_run + thr).any()) or bool(torch.isinf(m_run).any()):
                    m_run = torch.maximum(m_run, mt)
            n_main = min(n_full, nt - 1)
            j = 0
            if n_main > 0:
                mt = tile(raw, walk[0])
                m_true = torch.maximum(m_true, mt)
                lazily(mt)
                for jj in range(n_main):
                    mt = tile(raw, walk[jj + 1])                     # phase B: the maximum of S(jj + 1), unmasked
                    if jj + 1 < n_main or mutant == "nmain":
                        if not (mutant == "lost" and jj + 1 == lost):
                            m_true = torch.maximum(m_true, mt)
                    if jj + 1 < n_main:
                        lazily(mt)
                j = n_main
            for j in range(j, nt):
                if mutant == "lost" and j == lost:
                    continue
                mt = tile(raw if mutant == "nomask" else masked, walk[j])
                m_true = torch.maximum(m_true, mt)
                m_run = torch.maximum(m_run, mt)
            out[:, :, rows] = (m_run if mutant == "lazy" else m_true) * scale
    return out


def _white(B, Sq, Sk, Hq, Hkv, D, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, s, h, D, generator=g).to(torch.bfloat16) for s, h in ((Sq, Hq), (Sk, Hkv))]


def _needle(B, Sq, Sk, Hq, Hkv, D, seed, C=24):
    nd = NI.make(Sq, Sk, Hq, Hkv, D, "bfloat16", C, seed=seed, B=B)
    return [torch.from_numpy(x).to(torch.bfloat16) for x in (nd.q, nd.k)]


def _needle3(B, Sq, Sk, Hq, Hkv, D, seed):
    """Three classes: every row meets a needle of its class every third tile -- several per row at these lengths, their scores
    0.3 nat apart, so that the second one finds the reference already within 8 / c of it (the lazy trap)."""
    return _needle(B, Sq, Sk, Hq, Hkv, D, seed, C=3)


MODEL_CASES = [(320, 320, True, None, 4), (769, 769, True, None, 8), (129, 513, False, None, 4), (512, 512, True, (64, 0), 4),
               (64, 64, False, None, 4), (1, 65, False, None, 8)]


@pytest.mark.parametrize("inputs", [_white, _needle], ids=["white", "needle"])
@pytest.mark.parametrize("Sq,Sk,causal,window,waves", MODEL_CASES)
def test_model_of_the_walk_is_exact(inputs, Sq, Sk, causal, window, waves):
    """The walk as written folds every visible score exactly once and no hidden one: the model equals the reference bit for bit."""
    q, k = inputs(1, Sq, Sk, 4, 2, 128, 7)
    scale = 128 ** -0.5
    assert torch.equal(model_row_max(q, k, scale, causal, window, waves), R.row_max_ref(q, k, scale, causal, window))


def _miss(got, ref, scale, D, pairs):
    """The largest error as a multiple of the bound; a wrong -inf counts as a miss beyond any bound."""
    tol = R.tolerance(ref, scale, D, pairs)
    both = torch.isfinite(got) & torch.isfinite(ref)
    if not torch.equal(torch.isinf(got), torch.isinf(ref)):
        return float("inf")
    return float(((got - ref).abs() / tol)[both].max()) if bool(both.any()) else 0.0


@pytest.mark.parametrize("inputs", [_white, _needle3], ids=["white", "needle"])
def test_mutants_miss_the_bound(inputs):
    """Each trap, on N(0, 1) white noise and on needle inputs at D = 128: the mutant misses the derived bound by 2x or more (the
    honest model, checked beside it, sits at 0)."""
    D, scale = 128, 128 ** -0.5
    B, Hq, Hkv = 2, 4, 2
    seen = {}
    for Sq, Sk, causal, window, waves in ((320, 320, True, None, 4), (769, 769, True, None, 8), (769, 769, True, (300, 0), 8)):
        q, k = inputs(B, Sq, Sk, Hq, Hkv, D, 3)
        ref = R.row_max_ref(q, k, scale, causal, window)
        pairs = R.abs_pairs(q, k)
        assert _miss(model_row_max(q, k, scale, causal, window, waves), ref, scale, D, pairs) == 0.0
        for mutant in ("lazy", "nmain", "nomask", "lost"):
            m = _miss(model_row_max(q, k, scale, causal, window, waves, mutant), ref, scale, D, pairs)
            print(f"MAXLMUTANT {inputs.__name__} S{Sq} window={window} {mutant}: {m:.3g} x the bound")
            seen[mutant] = max(seen.get(mutant, 0.0), m)
            # (the window case, the rotated walk, is recorded: a 300-key window leaves a wave two or three pipelined tiles, which on
            # needle inputs hold one needle at most -- nothing for a lazy reference to miss)
            assert m >= 2.0 or window is not None, (mutant, Sq, window, m)
        # a merge that overwrites where it should take the maximum: keys [0, h) then [h, Sk), the second launch's value alone
        h = 256
        first = R.row_max_ref(q, k[:, :h], scale, causal, window, shift=(Sk - h))
        second = R.row_max_ref(q, k[:, h:], scale, causal, window)
        assert torch.equal(torch.maximum(first, second), ref)
        seen["overwrite"] = max(seen.get("overwrite", 0.0), _miss(second, ref, scale, D, pairs))
        # the wrong head's row: head h ^ 1 of the same KV group
        seen["head"] = max(seen.get("head", 0.0), _miss(ref[:, [1, 0, 3, 2]], ref, scale, D, pairs))
    assert all(v >= 2.0 for v in seen.values()), seen


def test_lazy_reference_sits_several_units_low():
    """What the issue states: m_run * scale can sit up to 8 / log2(e) = 5.5 score units under the true maximum, on plain white
    noise at D = 128 it is units, not rounding."""
    q, k = _white(2, 769, 769, 4, 2, 128, 3)
    scale = 128 ** -0.5
    gap = R.row_max_ref(q, k, scale, True) - model_row_max(q, k, scale, True, None, 8, "lazy")
    assert 0.0 <= float(gap.min()) and 1.0 < float(gap.max()) <= 8.0 / LOG2E + 1e-9, (float(gap.min()), float(gap.max()))


# ---- 2. the C ABI -------------------------------------------------------------------------------------------------------------------
def _lib():
    from yunchang_amd import _C
    if not os.path.exists(_C.lib_path()):
        pytest.fail("libusp_hip.so is not built: run __graft_entry__.build() first")
    return _C, _C.load()


def _args(_C, addr):
    a = _C.UspFwdArgs()
    a.dtype, a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D = 0, 1, 16, 16, 2, 2, 128
    a.softmax_scale = 0.125
    a.lse = addr
    a.q.ptr = a.k.ptr = a.v.ptr = a.out.ptr = a.acc.ptr = addr
    a.final_end = a.Sq
    for t in (a.q, a.k, a.v, a.out, a.acc):
        t.stride_b, t.stride_s, t.stride_h = 16 * 2 * 128, 2 * 128, 128
    return a


def test_abi_feature_bit_and_entry_points():
    _C, L = _lib()
    txt = open(os.path.join(ROOT, "include", "usp_hip.h")).read()
    assert _C.USP_ATTN_MAX_LOGIT == 16384 == int(re.search(r"#define USP_ATTN_MAX_LOGIT (\d+)", txt).group(1))
    assert _C.USP_ATTN_MAX_LOGIT == 2 * _C.USP_ATTN_BLOCK_MASK                       # the next free bit
    assert L.usp_attn_features() & _C.USP_ATTN_MAX_LOGIT
    assert L.usp_attn_features() & 0x3fc2 == 0x3fc2                                  # ... and every earlier one still
    assert L.usp_abi_version() == 7 == _C.ABI_VERSION
    for name in ("usp_flash_fwd_maxlogit", "usp_row_max_reduce"):
        assert name in _C.MAXL_EXPORTS and name in _C.EXPORTS and hasattr(L, name)
        assert _C._maxl_entry(name).restype is ctypes.c_int
    assert _C._maxl_entry("usp_flash_fwd_maxlogit").argtypes[1:] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    assert len(_C._maxl_entry("usp_row_max_reduce").argtypes) == 9
    assert re.search(r"int usp_flash_fwd_maxlogit\(const usp_fwd_args\* args, float\* row_max, int64_t row_max_stride_b, "
                     r"int64_t row_max_stride_h,\s+void\* stream\);", txt)
    assert ctypes.sizeof(_C.UspFwdArgs) == 296 and ctypes.sizeof(_C.UspBwdArgs) == 504      # the argument blocks are unchanged


def test_abi_declines_without_launch(monkeypatch):
    """Host memory stands in for the device pointers: every call below returns before anything is launched."""
    _C, L = _lib()
    fwd, red = _C._maxl_entry("usp_flash_fwd_maxlogit"), _C._maxl_entry("usp_row_max_reduce")
    buf = ctypes.create_string_buffer(1 << 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    rm = addr + 4096
    seq = (ctypes.c_int32 * 2)(0, 16)
    a = _args(_C, addr)
    assert fwd(ctypes.byref(a), rm, -1, 16, None) == -1 and fwd(ctypes.byref(a), rm, 32, -16, None) == -1      # a negative stride
    a.flags, a.softcap = _C.USP_ATTN_SOFTCAP, 30.0
    assert fwd(ctypes.byref(a), rm, 32, 16, None) == -2
    a = _args(_C, addr)                            # a packed batch
    a.seq_q = a.seq_k = ctypes.addressof(seq)
    assert fwd(ctypes.byref(a), rm, 32, 16, None) == -2
    a = _args(_C, addr)                            # the 64-row family forced
    a.flags = _C.USP_FORCE_ROW64
    assert fwd(ctypes.byref(a), rm, 32, 16, None) == -2
    a = _args(_C, addr)                            # the existing checks still come first
    a.flags, a.softmax_scale = _C.USP_FORCE_ROW64, 0.0
    assert fwd(ctypes.byref(a), rm, 32, 16, None) == -1
    a = _args(_C, addr)
    a.flags, a.D = _C.USP_FORCE_ROW64, 96
    assert fwd(ctypes.byref(a), rm, 32, 16, None) == -2
    # row_max == NULL is exactly usp_flash_fwd, whatever the strides: the plain path's own checks answer
    a = _args(_C, addr)
    a.merge_in, a.acc.ptr = 1, None
    assert fwd(ctypes.byref(a), None, -5, -5, None) == L.usp_flash_fwd(ctypes.byref(a), None) == -1
    a = _args(_C, addr)
    a.flags, a.D = _C.USP_FORCE_ROW64, 64
    assert fwd(ctypes.byref(a), None, 0, 0, None) == L.usp_flash_fwd(ctypes.byref(a), None) == -2
    assert L.usp_last_launch_kinds() == 0
    assert bytes(buf) == bytes(1 << 16)            # nothing written
    # usp_row_max_reduce: null pointers, non-positive sizes, negative strides
    for bad in ((0, 4, 2, rm, 8, 4, addr), (1, 0, 2, rm, 8, 4, addr), (1, 4, 0, rm, 8, 4, addr), (1, 4, 2, None, 8, 4, addr),
                (1, 4, 2, rm, 8, 4, None), (1, 4, 2, rm, -8, 4, addr), (1, 4, 2, rm, 8, -4, addr)):
        B, S, H, p, sb, sh, o = bad
        assert red(B, S, H, p, sb, sh, o, 0, None) == -1, bad

    # a library without the feature bit
    class Old:
        @staticmethod
        def usp_attn_features():
            return 0x3fc2
    monkeypatch.setattr(_C, "load", lambda: Old)
    with pytest.raises(NotImplementedError, match="rebuild it"):
        _C._maxl_entry("usp_flash_fwd_maxlogit")


# ---- 3. Python: refusals ------------------------------------------------------------------------------------------------------------
def test_refusal_matrix():
    import yunchang_amd as Y
    from yunchang_amd import _C
    from yunchang_amd.kernels import attention as KA
    from yunchang_amd.kernels.features import max_logits_alone
    from yunchang_amd.ring.ring_flash_attn_varlen import ring_flash_attn_varlen_func
    from yunchang_amd.ring.zigzag_ring_flash_attn_varlen import zigzag_ring_flash_attn_varlen_func
    q = torch.zeros(2, 128, 4, 64, dtype=torch.bfloat16, device="meta")      # (meta: a refusal that read a tensor would fail)
    others = (("softcap", 30.0), ("alibi_slopes", torch.rand(4)), ("dropout_p", 0.1), ("sinks", torch.rand(4)),
              ("cu_doclens", [0, 64, 128]), ("bidirectional", [(0, 8)]), ("block_mask", torch.ones(1, 1, dtype=torch.bool)))
    for name, value in others:
        kw = {name: value}
        for call in (lambda: KA.hip_attn_forward(q, q, q, causal=True, return_max_logits=True, **kw),
                     lambda: KA.hip_attn_func(q, q, q, causal=True, return_max_logits=True, **kw),
                     lambda: Y.ring_flash_attn_func(q, q, q, causal=True, return_max_logits=True, **kw),
                     lambda: Y.zigzag_ring_flash_attn_func(q, q, q, causal=True, return_max_logits=True, **kw),
                     lambda: Y.stripe_flash_attn_func(q, q, q, causal=True, return_max_logits=True, **kw),
                     lambda: Y.ring_flash_attn_kvpacked_func(q, torch.stack([q, q], 2), causal=True, return_max_logits=True, **kw),
                     lambda: Y.zigzag_ring_flash_attn_qkvpacked_func(torch.stack([q, q, q], 2), causal=True, return_max_logits=True, **kw)):
            with pytest.raises(NotImplementedError, match="return_max_logits together with " + name):
                call()
        assert max_logits_alone(False, **kw) is False and max_logits_alone(None, **kw) is False      # off: judged not at all
    assert max_logits_alone(True) is True and max_logits_alone(True, softcap=0.0, dropout_p=0.0) is True
    # the launch itself takes no second extra either
    with pytest.raises(NotImplementedError, match="row_max together with sinks"):
        _C._flash_call("fwd", None, None, None, torch.rand(4), None, None, mx=(None, 0, 0))
    # the variable-length rings refuse and name the dense functions
    t3 = torch.zeros(32, 4, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 32], dtype=torch.int32)
    for f in (ring_flash_attn_varlen_func, zigzag_ring_flash_attn_varlen_func):
        with pytest.raises(NotImplementedError, match="packed.*ring_flash_attn_func"):
            f(t3, t3, t3, cu, 32, causal=True, return_max_logits=True)
    # the value of row_max is checked before a device is touched
    for bad in (torch.zeros(2, 4, 128), torch.zeros(2, 4, 128, dtype=torch.float64).to(torch.float16), [0.0]):
        with pytest.raises(ValueError):
            _C.row_max_value(bad, 2, 4, 127, torch.device("cpu"))


def test_row_max_backend_shadows_the_lse():
    """RowMaxBackend: a launch gets the view of the shadow that its lse is of its storage; `merge` combines the maxima."""
    from yunchang_amd.kernels import attention as KA
    seen = []

    class Rec:
        def fwd(self, q, k, v, scale, causal, lse, *a, **kw):
            seen.append((kw["row_max"], a, {n: x for n, x in kw.items() if n != "row_max"}))

        def merge(self, *a):
            seen.append("merge")

        def row_max_reduce(self, rm, out=None, accum=False):
            return rm.amax(dim=(0, 2))

        def add(self):
            return "add"
    be = KA.RowMaxBackend(Rec())
    lse, blk = torch.zeros(2, 4, 64), torch.zeros(2, 4, 64)
    be.fwd(0, 1, 2, 3, True, lse, "out", window=(3, 0))
    be.fwd(0, 1, 2, 3, False, lse[:, :, 32:], "out", "acc", True)
    whole, part = seen[0][0], seen[1][0]
    assert whole.shape == lse.shape and whole.stride() == lse.stride() and whole.dtype == torch.float32
    assert part.shape == (2, 4, 32) and part.data_ptr() == whole[:, :, 32:].data_ptr() and part.stride() == whole.stride()
    assert seen[0][1:] == (("out",), {"window": (3, 0)}) and seen[1][1:] == (("out", "acc", True), {})
    whole.copy_(torch.arange(2 * 4 * 64, dtype=torch.float32).view(2, 4, 64))
    assert torch.equal(be.max_logits(lse), whole.amax(dim=(0, 2)))
    be.fwd(0, 1, 2, 3, False, blk)
    seen[-1][0].fill_(1000.0)
    seen[-1][0][:, 0] = -1.0
    be.merge("acc", lse, "o", blk, False)
    assert bool((whole[:, 1:] == 1000.0).all()) and bool((whole[:, 0] >= 0).all())
    be.merge("acc", lse, "o", blk, True)
    assert bool((whole[:, 0] == -1.0).all())
    assert be.add() == "add"


# ---- 4. the schedules on gloo -------------------------------------------------------------------------------------------------------
B, H, D, CH = 2, 4, 32, 32                # CH rows per rank (even: the zigzag layout)
SCALE = D ** -0.5
IMPLS = ("basic", "zigzag", "strip")


def _inputs(ws, hkv):
    g = torch.Generator().manual_seed(11 + hkv)
    S = CH * ws
    return [torch.randn(B, S, h, D, generator=g).to(torch.bfloat16) for h in (H, hkv, hkv, H)]


def _share(layer_call, loc, be, backward=True):
    """(out with the keyword, out without, this rank's share, calls with, calls without, row_max calls without)"""
    del be.calls[:], be.row_max_calls[:]
    ts = [t.detach().clone().requires_grad_(True) for t in loc[:-1]]
    plain = layer_call(*ts, False)
    plain.backward(loc[-1])
    calls0, rm0 = list(be.calls), list(be.row_max_calls)
    g0 = [t.grad.clone() for t in ts]
    del be.calls[:], be.row_max_calls[:]
    ts = [t.detach().clone().requires_grad_(True) for t in loc[:-1]]
    out, ml = layer_call(*ts, True)
    assert ml.dtype == torch.float32 and not ml.requires_grad
    out.backward(loc[-1])
    same = torch.equal(out, plain) and all(torch.equal(a, t.grad) for a, t in zip(g0, ts))
    reduces = [c for c in be.row_max_calls if c[0] == "reduce"]
    return ml.clone(), same, calls0 == list(be.calls), rm0 == [], len(reduces)


def _grid_worker(rank, ws, ud, rd):
    import yunchang_amd as Y
    from yunchang_amd.kernels import set_block_backend
    be = R.MaxLogitOracleBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    os.environ.pop("USP_RING_WINDOW", None)
    # the keyword takes the three-exchange path, as every feature does: the call without it is held to the same structure here, so
    # that its launches and bits are the ones to compare with (USP_PACK_QKV=0: the documented A/B switch)
    os.environ["USP_PACK_QKV"] = "0"
    res = {}
    for impl in IMPLS:
        ext = Y.EXTRACT_FUNC_DICT[impl]
        loc = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in _inputs(ws, 2)]
        attn = Y.LongContextAttention(ring_impl_type=impl)
        res[(impl, "layer")] = _share(lambda q, k, v, on: attn(q, k, v, causal=True, return_max_logits=on), loc, be)
        lq, lk, lv, ldo = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in _inputs(ws, H)]
        packed = Y.LongContextAttentionQKVPacked(ring_impl_type=impl)
        res[(impl, "packed")] = _share(lambda qkv, on: packed(qkv, causal=True, return_max_logits=on),
                                       [torch.stack([lq, lk, lv], dim=2), ldo], be)
    if ud == 1:                                    # the kv-packed function of every ring, straight
        for impl, fn in (("basic", Y.ring_flash_attn_kvpacked_func), ("zigzag", Y.zigzag_ring_flash_attn_kvpacked_func),
                         ("strip", Y.stripe_flash_attn_kvpacked_func)):
            ext = Y.EXTRACT_FUNC_DICT[impl]
            lq, lk, lv, ldo = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in _inputs(ws, 2)]
            out, lse, none, ml = fn(lq, torch.stack([lk, lv], dim=2), causal=True, return_attn_probs=True, return_max_logits=True)
            assert none is None and lse.shape == (B, H, lq.shape[1])
            res[(impl, "kvpacked")] = (ml.clone(), True, True, True, 1)
    try:                                           # the async layer refuses and names the layer that serves it
        Y.AsyncLongContextAttention(ring_impl_type="basic")(*loc[:3], causal=True, return_max_logits=True)
        res["async"] = False
    except NotImplementedError as e:
        res["async"] = "LongContextAttention" in str(e)
    return res


@pytest.mark.parametrize("ws,ud,rd", [(2, 1, 2), (4, 1, 4), (2, 2, 1), (4, 2, 2)])
def test_rings_and_layers_on_gloo(ws, ud, rd):
    """Each rank's share: its rows of the ring, its heads under Ulysses (-inf exactly elsewhere); the MAX over the ranks is the
    single-process value -- exactly: the oracle's fp64 maxima rounded to fp32, and rounding is monotone.  out and the gradients are
    those of the call without the keyword, whose backend calls are as they ever were; one reduce per call."""
    from yunchang_amd.comm.all_to_all import local_heads
    res = run_distributed(_grid_worker, ws, ud, rd)
    for kind, hkv in (("layer", 2), ("packed", H)) + ((("kvpacked", 2),) if ud == 1 else ()):
        q, k = _inputs(ws, hkv)[:2]
        want = R.max_logits_ref(q, k, SCALE, True).to(torch.float32)
        for impl in IMPLS:
            shares = []
            for rank in range(ws):
                ml, same, calls_same, no_rm, reduces = res[rank][(impl, kind)]
                assert same and calls_same and no_rm and reduces == 1, (impl, kind, rank, same, calls_same, no_rm, reduces)
                assert ml.shape == (H,)
                mine = torch.zeros(H, dtype=torch.bool)
                mine[local_heads(H, ud, rank % ud)] = True
                assert bool((ml[~mine] == float("-inf")).all()) and bool(torch.isfinite(ml[mine]).all()), (impl, kind, rank, ml)
                shares.append(ml)
            assert torch.equal(torch.stack(shares).amax(0), want), (impl, kind, torch.stack(shares), want)
            if rd > 1:                             # a ring rank alone does not hold the maximum of every head (the contract is a MAX)
                assert any(not torch.equal(torch.where(torch.isinf(s), want, s), want) for s in shares), (impl, kind)
    assert all(r["async"] is True for r in res)


def _ulysses_worker(rank, ws):
    import torch.distributed as dist
    import yunchang_amd as Y
    from yunchang_amd.kernels import set_block_backend
    be = R.MaxLogitOracleBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ws, 1, rank, ws)
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    loc = [ext(t, rank, world_size=ws, rd=1, ud=ws).detach().clone() for t in _inputs(ws, 2)]
    layer = Y.UlyssesAttention(dist.group.WORLD, attn_type=Y.AttnType.HIP)
    res = {}
    for name, kw in (("causal", dict(causal=True)), ("window", dict(causal=True, window_size=(20, 0))), ("full", dict(causal=False))):
        res[name] = _share(lambda q, k, v, on: layer(q, k, v, return_max_logits=on, **kw), loc, be)
    return res


def test_ulysses_layer_on_gloo():
    from yunchang_amd.comm.all_to_all import local_heads
    ws = 2
    res = run_distributed(_ulysses_worker, ws)
    q, k = _inputs(ws, 2)[:2]
    for name, causal, window in (("causal", True, None), ("window", True, (20, 0)), ("full", False, None)):
        want = R.max_logits_ref(q, k, SCALE, causal, window).to(torch.float32)
        shares = []
        for rank in range(ws):
            ml, same, calls_same, no_rm, reduces = res[rank][name]
            assert same and calls_same and no_rm and reduces == 1, (name, rank)
            mine = torch.zeros(H, dtype=torch.bool)
            mine[local_heads(H, ws, rank)] = True
            assert bool((ml[~mine] == float("-inf")).all()) and torch.equal(ml[mine], want[mine]), (name, rank, ml, want)
            shares.append(ml)
        assert torch.equal(torch.stack(shares).amax(0), want)


def _window_worker(rank, ws):
    import yunchang_amd as Y
    from test_ring_window_cpu import ShiftOracleBackend
    from yunchang_amd.kernels import set_block_backend

    class WindowBackend(R.MaxLogitOracleBackend, ShiftOracleBackend):
        """row_max= in front of the oracle that takes `shift`"""
    be = WindowBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(1, ws, rank, ws)
    os.environ["USP_RING_WINDOW"] = "global"
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    lq, lk, lv, ldo = [ext(t, rank, world_size=ws, rd=ws, ud=1).detach().clone() for t in _inputs(ws, 2)]
    res = {}
    for window in ((20, 0), (40, 8), (5, 70)):
        out, ml = Y.ring_flash_attn_func(lq, lk, lv, causal=False, window_size=window, return_max_logits=True)
        res[window] = (ml.clone(), torch.equal(out, Y.ring_flash_attn_func(lq, lk, lv, causal=False, window_size=window)))
    return res


@pytest.mark.parametrize("ws", [2, 4])
def test_basic_ring_with_the_global_window_on_gloo(ws):
    res = run_distributed(_window_worker, ws)
    q, k = _inputs(ws, 2)[:2]
    for window in ((20, 0), (40, 8), (5, 70)):
        want = R.max_logits_ref(q, k, SCALE, False, window).to(torch.float32)
        assert all(r[window][1] for r in res)
        assert torch.equal(torch.stack([r[window][0] for r in res]).amax(0), want), window
