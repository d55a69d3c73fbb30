"""Every element of the flash kernels at multi-pass launch sizes, against exact fp64 attention computed on the GPU.

Every flash launch is persistent: at most one workgroup per CU (two 4-wave forward workgroups per CU), each walking a
static list of work items pass after pass, cut into eight per-XCD runs and reordered by usp_item_deal.h where 8 divides
both counts.  The dealing of fewer than 8 heads (regular and irregular), the KV-group walk, the automatic dK/dV head
grouping, the automatic K split and backward cuts, and the overlap of one item's loads with the previous item's epilogue
(usp_common.hpp ItemWalk) only run when a launch has more items than workgroups -- which no small shape of the other
GPU files reaches, and which production always runs.  Here every case:

- declares the kernel kinds it must run (asserted from `_C.last_launch_kinds()`) and asserts that each of its flash
  launches is multi-pass (item count above the resident workgroups, counted from the shape and the binding's own
  `fwd_k_splits` / `bwd_splits` / the library's workspace size);
- keeps its 16-bit operands and NaN-prefilled outputs in a NaN arena with guard bands (test_gpu_row64._Arena);
- compares every element of out / lse and of dq / dk / dv with tests/attn_ref_torch.py (fp64, on the device);
- runs every launch twice (bit-identical) and once more with `interleave=True` (one workgroup per item): bit-identical
  where the same kernels run, within tolerance otherwise.

USP_LARGE_ALL=1 adds the bench shape in full, larger variants and fp16 variants.
"""
import contextlib
import ctypes
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np
import pytest
import torch

from attn_ref_torch import ref_bwd, ref_delta, ref_fwd
from golden_util import TOL, assert_close, long_sum_atol

pytestmark = pytest.mark.gpu

_ALL = os.environ.get("USP_LARGE_ALL", "0") == "1"


class Case(NamedTuple):
    id: str
    B: int
    Sq: int
    Sk: int
    Hq: int
    Hkv: int
    D: int
    causal: bool
    dt: str
    fwd: Tuple[str, ...]                  # kinds the forward must run
    bwd: Tuple[str, ...]                  # kinds the backward must run
    gsub: int                             # query heads per dK/dV item the library picks (dkdv_heads = 0)
    window: Optional[Tuple[int, int]] = None
    softcap: Optional[float] = None
    q_mul: float = 1.0
    k_mul: float = 1.0
    k_splits: Optional[int] = None        # None: the binding's fwd_k_splits decides
    seed: int = 0


_R64 = ("dkdv_row64", "dq_row64")
_W8 = ("dkdv_wave8", "dq_wave8")
CASES = [
    Case("A", 1, 8192, 8192, 16, 2, 128, True, "bfloat16", ("fwd_row64",), _R64 + ("reduce_heads",), 2),
    Case("B", 1, 32768, 32768, 4, 1, 128, True, "bfloat16", ("fwd_row64",), _R64 + ("reduce_heads",), 2, k_splits=0),
    Case("C", 1, 16384, 16384, 6, 2, 128, True, "bfloat16", ("fwd_row64", "fwd_split_merge"),
         _R64 + ("reduce_heads", "reduce_cuts"), 1),
    Case("D", 2, 8192, 8192, 16, 4, 64, True, "bfloat16", ("fwd_wave8",), _W8 + ("reduce_heads",), 2),
    # q x 4 and k x 4 (exact in 16 bits), as test_gpu_softcap's cap30 case: scores reach ~70, so the cap 30 bites
    Case("E", 1, 8192, 8192, 16, 2, 128, True, "bfloat16", ("fwd_wave8",), _W8 + ("reduce_heads",), 2, softcap=30.0,
         q_mul=4.0, k_mul=4.0),
    Case("E2", 1, 16384, 16384, 6, 2, 128, True, "bfloat16", ("fwd_wave8", "fwd_split_merge"),
         _W8 + ("reduce_heads", "reduce_cuts"), 1, softcap=3.0, q_mul=4.0),
    Case("F", 1, 16384, 16384, 8, 4, 128, True, "bfloat16", ("fwd_wave8",), _W8, 2, window=(4096, 0)),
    Case("G", 1, 6144, 12288, 16, 2, 128, False, "float16", ("fwd_row64",), _R64 + ("reduce_heads",), 4),
    Case("H", 3, 9000, 9000, 5, 1, 128, True, "bfloat16", ("fwd_row64",), _R64 + ("reduce_heads",), 1),
    Case("I", 1, 32768, 32768, 4, 2, 128, True, "bfloat16", ("fwd_row64",), _R64, 2),
    Case("J", 8, 1024, 1024, 32, 8, 128, True, "bfloat16", ("fwd_wave4",), _R64 + ("reduce_heads",), 2),
    Case("K", 4, 8192, 8192, 8, 8, 32, False, "bfloat16", ("fwd_wave8",), _W8, 1),
    Case("L", 1, 16384, 8192, 8, 1, 128, True, "bfloat16", ("fwd_row64",), _R64 + ("reduce_heads",), 1),
]
_BY_ID = {c.id: c for c in CASES}
LARGE = [
    Case("bench", 1, 65536, 65536, 32, 4, 128, True, "bfloat16", ("fwd_row64",), _R64 + ("reduce_heads",), 2),
    _BY_ID["A"]._replace(id="A16k", Sq=16384, Sk=16384),
    _BY_ID["B"]._replace(id="B64k", Sq=65536, Sk=65536),
] + [_BY_ID[i]._replace(id=i + "-fp16", dt="float16") for i in ("A", "B", "C", "D", "E", "E2", "F")]


def _cus(dev=None):
    if dev is None:
        return 256
    return torch.cuda.get_device_properties(dev).multi_processor_count


def fwd_launch(case, cus=256, interleave=False):
    """(kind, n_items, resident slots, n_inner, ksplit) of the forward flash launch of `case`, from the declared kinds,
    the shape and the binding's own K-split policy (usp_flash_fwd.hip launch_fwd / launch_fwd_w, usp_flash_fwd64.hip)."""
    from yunchang_amd import _C
    kind = next(k for k in case.fwd if k != "fwd_split_merge")
    n = _C.fwd_k_splits(case.B, case.Sq, case.Hq, case.causal) if case.k_splits is None else case.k_splits
    ks = n if n > 1 else 1
    assert ("fwd_split_merge" in case.fwd) == (ks > 1), (case.id, ks)
    rows = 128 if kind == "fwd_wave4" else 256
    nq = -(-case.Sq // rows)
    slots = cus * (2 if kind == "fwd_wave4" else 1)
    return kind, case.B * case.Hq * nq * ks, slots, nq * ks if ks > 1 else nq, ks


def dq_launch(case, cus=256):
    """(kind, n_items, slots, n_inner, ksplit) of the dQ launch (usp_flash_bwd.hip launch_bwd, usp_flash_bwd_dq64.hip)."""
    from yunchang_amd import _C
    kind = next(k for k in case.bwd if k.startswith("dq_"))
    dqs = _C.bwd_splits(case.B, case.Sq, case.Sk, case.Hq, case.causal)[0]
    ks = dqs if dqs > 1 else 1
    assert ("reduce_cuts" in case.bwd) == (ks > 1), (case.id, ks)
    nblk = -(-case.Sq // 256)
    return kind, case.B * case.Hq * nblk * ks, cus, nblk, ks


def dkdv_launch(case, cus=256):
    """(kind, n_items, slots) of the dK/dV launch: B * Hkv * ceil(Sk / 128) * (G / heads per item) * cuts."""
    from yunchang_amd import _C
    kind = next(k for k in case.bwd if k.startswith("dkdv_"))
    G = case.Hq // case.Hkv
    cuts = _C.bwd_splits(case.B, case.Sq, case.Sk, case.Hq, case.causal)[1]
    split = G // case.gsub > 1 or cuts > 1
    assert ("reduce_heads" in case.bwd) == split, (case.id, case.gsub, cuts)
    n = case.B * case.Hkv * -(-case.Sk // 128) * ((G // case.gsub) * max(1, cuts) if split else 1)
    return kind, n, cus


def _bwd_workspace_bytes(case, dkdv_heads=0, splits=None):
    """What the library asks for (usp_flash_bwd_workspace_bytes) for this case: pins the automatic dkdv_heads."""
    from yunchang_amd import _C
    a = _C.UspBwdArgs()
    a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D = case.B, case.Sq, case.Sk, case.Hq, case.Hkv, case.D
    a.causal = int(case.causal)
    if case.window is not None:
        a.flags |= _C.USP_ATTN_WINDOW
        a.window_left, a.window_right = case.window
    a.dq_splits, a.dkdv_splits = _C.bwd_splits(case.B, case.Sq, case.Sk, case.Hq, case.causal) if splits is None else splits
    a.dkdv_heads = dkdv_heads
    return _C.load().usp_flash_bwd_workspace_bytes(ctypes.byref(a))


def _expected_ws(case, gsub, dq_splits, dkdv_splits):
    G = case.Hq // case.Hkv
    slabs = (G // gsub) * max(1, dkdv_splits)
    part = 2 * slabs * case.B * case.Sk * case.Hkv * case.D * 4 if slabs > 1 else 0
    return part + (dq_splits * case.B * case.Sq * case.Hq * case.D * 4 if dq_splits > 1 else 0)


@pytest.fixture(scope="module")
def dev():
    from yunchang_amd import _C
    _C.load()
    return torch.device("cuda:0")


def _inputs(case, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + case.seed)
    dt = getattr(torch, case.dt)
    qs, ks = (case.B, case.Sq, case.Hq, case.D), (case.B, case.Sk, case.Hkv, case.D)
    q = (torch.randn(qs, generator=gen, device=dev) * case.q_mul).to(dt)
    k = (torch.randn(ks, generator=gen, device=dev) * case.k_mul).to(dt)
    v = torch.randn(ks, generator=gen, device=dev).to(dt)
    do = torch.randn(qs, generator=gen, device=dev).to(dt)
    return q, k, v, do


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _empty_rows(rl):
    """(B,Hq,Sq) lse -> (B,Sq,Hq,1) bool: rows without a visible key."""
    return ~torch.isfinite(rl).transpose(1, 2)[..., None]


def _check_fwd(what, out, lse, ro, rl, dt):
    fin = torch.isfinite(rl)
    assert torch.equal(torch.isfinite(lse), fin), what + ": rows without a visible key must give lse = -inf (and only they)"
    assert_close(out, ro, *TOL[dt]["out"], what + " out")
    assert_close(lse[fin], rl[fin], 2e-3, 1e-4, what + " lse")
    empty = _empty_rows(rl).expand_as(out)
    assert bool((out[empty] == 0).all()), what + ": rows without a visible key must give out = 0"


def _check_bwd(what, grads, refs, case):
    G = case.Hq // case.Hkv
    for g_, r_, n_ in zip(grads, refs, ("dq", "dk", "dv")):
        atol, rtol = TOL[case.dt]["grad"]
        atol = long_sum_atol(atol, case.Sk if n_ == "dq" else case.Sq * G, r_)
        assert_close(g_, r_, atol, rtol, f"{what} {n_}")


_REF = {}


def _reference(case, dev, inputs=None):
    """Inputs and the fp64 reference of a case (cached per process: the sweep tests share theirs).  `inputs`: another
    source of (q, k, v, do) than the seeded N(0,1) draw -- a function of (case, dev) with a `__name__` (the cache key)."""
    key = case.id if inputs is None else (case.id, inputs.__name__)
    if key not in _REF:
        _REF.clear()
        q, k, v, do = (_inputs if inputs is None else inputs)(case, dev)
        scale = case.D ** -0.5
        ro, rl = ref_fwd(q, k, v, scale, case.causal, case.window, case.softcap)
        o16 = ro.to(q.dtype)
        rdq, rdk, rdv, delta = ref_bwd(do, q, k, v, o16, rl, scale, case.causal, case.window, case.softcap)
        _REF[key] = dict(q=q, k=k, v=v, do=do, ro=ro, rl=rl, o16=o16, grads=(rdq, rdk, rdv), delta=delta)
    return _REF[key]


def _assert_cap_bites(case, r):
    """The capped and the uncapped exact outputs differ by more than the tolerance: the case tests the cap."""
    ro0, _ = ref_fwd(r["q"], r["k"], r["v"], case.D ** -0.5, case.causal, case.window, None)
    diff = float((ro0 - r["ro"]).abs().max())
    assert diff > 10 * TOL[case.dt]["out"][0], f"{case.id}: the cap does not bite (max |capped - uncapped| = {diff:.3e})"


def run_case(dev, case, inputs=None):
    """`inputs` = None: the seeded N(0,1) draw of `_inputs`; tests/test_gpu_needle.py passes its needle source."""
    from yunchang_amd import _C
    cus = _cus(dev)
    what = f"{case.id}: B{case.B} Sq{case.Sq} Sk{case.Sk} Hq{case.Hq} Hkv{case.Hkv} D{case.D} causal={case.causal} " \
           f"{case.dt} window={case.window} softcap={case.softcap}"
    # ---- every launch is multi-pass --------------------------------------------------------------------------------
    fk, fn, fslots, _, _ = fwd_launch(case, cus)
    qk, qn, qslots, _, qks = dq_launch(case, cus)
    kk, kn, kslots = dkdv_launch(case, cus)
    assert fn > fslots and qn > qslots and kn > kslots, (what, (fk, fn, fslots), (qk, qn, qslots), (kk, kn, kslots))
    cuts = _C.bwd_splits(case.B, case.Sq, case.Sk, case.Hq, case.causal)
    assert _bwd_workspace_bytes(case) == _expected_ws(case, case.gsub, *cuts), (what, "dkdv_heads", case.gsub)
    r = _reference(case, dev, inputs)
    if case.softcap:
        _assert_cap_bites(case, r)
    dt, scale = case.dt, case.D ** -0.5
    qs, ks = tuple(r["q"].shape), tuple(r["k"].shape)
    from test_gpu_row64 import _Arena
    ar = _Arena(dt, dev, [qs, ks, ks, qs] + [qs] * 3 + [qs, ks, ks] * 3)
    tq, tk, tv, tdo = (ar.put(r[n]) for n in ("q", "k", "v", "do"))
    kw = dict(window=case.window, softcap=case.softcap)
    # ---- forward ---------------------------------------------------------------------------------------------------
    fwd = []
    for interleave in (False, False, True):
        out = ar.out(qs)
        lse = torch.full((case.B, case.Hq, case.Sq), float("nan"), dtype=torch.float32, device=dev)
        _C.flash_fwd(tq, tk, tv, scale, case.causal, lse, out=out, interleave=interleave, k_splits=case.k_splits, **kw)
        fwd.append((out, lse, _C.last_launch_kinds()))
    assert set(fwd[0][2]) == set(case.fwd), (what, fwd[0][2])
    _check_fwd(what, fwd[0][0], fwd[0][1], r["ro"], r["rl"], dt)
    assert fwd[1][2] == fwd[0][2] and _same_bits(fwd[1][0], fwd[0][0]) and _same_bits(fwd[1][1], fwd[0][1]), \
        what + ": two persistent forward launches differ"
    if fwd[2][2] == fwd[0][2]:
        assert _same_bits(fwd[2][0], fwd[0][0]) and _same_bits(fwd[2][1], fwd[0][1]), \
            what + ": the interleaved forward launch differs from the persistent one"
    else:
        _check_fwd(what + f" (interleaved: {fwd[2][2]})", fwd[2][0], fwd[2][1], r["ro"], r["rl"], dt)
    # ---- backward (exact lse, delta from the 16-bit-rounded reference out) ----------------------------------------
    lse_t = r["rl"].float().contiguous()
    delta_t = r["delta"].float().contiguous()
    bwd = []
    for interleave in (False, False, True):
        dq, dk, dv = ar.out(qs), ar.out(ks), ar.out(ks)
        _C.flash_bwd(tdo, tq, tk, tv, lse_t, delta_t, None, None, None, scale, case.causal, dq16=dq, dk16=dk, dv16=dv,
                     interleave=interleave, **kw)
        bwd.append(((dq, dk, dv), _C.last_launch_kinds()))
    assert set(bwd[0][1]) == set(case.bwd), (what, bwd[0][1])
    _check_bwd(what, bwd[0][0], r["grads"], case)
    empty = _empty_rows(r["rl"]).expand_as(bwd[0][0][0])
    assert bool((bwd[0][0][0][empty] == 0).all()), what + ": rows without a visible key must give dq = 0"
    assert bwd[1][1] == bwd[0][1] and all(_same_bits(a, b) for a, b in zip(bwd[1][0], bwd[0][0])), \
        what + ": two persistent backward launches differ"
    if bwd[2][1] == bwd[0][1]:
        assert all(_same_bits(a, b) for a, b in zip(bwd[2][0], bwd[0][0])), \
            what + ": the interleaved backward launches differ from the persistent ones"
    else:
        _check_bwd(what + f" (interleaved: {bwd[2][1]})", bwd[2][0], r["grads"], case)
    assert ar.guards_intact(), what + ": a launch wrote outside its tensors"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_large_launch(dev, case):
    run_case(dev, case)


@pytest.mark.skipif(not _ALL, reason="USP_LARGE_ALL=1 runs the larger set")
@pytest.mark.parametrize("case", LARGE, ids=[c.id for c in LARGE])
def test_large_launch_all(dev, case):
    run_case(dev, case)


# ---------------------------------------------------------------------------------------------------------------------
# dkdv_heads (ABI v7) and the workspace contract: B2 S16384 H16/Hkv2 causal (G = 8), every setting multi-pass
# ---------------------------------------------------------------------------------------------------------------------
SWEEP = Case("sweep", 2, 16384, 16384, 16, 2, 128, True, "bfloat16", (), (), 2, seed=7)


class _WorkspaceProxy:
    """Stands in for the loaded library inside _C.flash_bwd and hands usp_flash_bwd a workspace of its own: none, one byte
    short of what usp_flash_bwd_workspace_bytes asks for, or one that is not 16-byte aligned."""

    def __init__(self, lib, mode, dev):
        self._lib, self._mode, self._dev, self.need = lib, mode, dev, None

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def usp_flash_bwd(self, aref, stream):
        a = aref._obj
        self.need = need = int(self._lib.usp_flash_bwd_workspace_bytes(aref))
        assert need > 0
        if self._mode == "none":
            a.workspace, a.workspace_bytes = None, 0
            return self._lib.usp_flash_bwd(aref, stream)
        buf = torch.empty(need + 64, dtype=torch.uint8, device=self._dev)
        if self._mode == "short":
            a.workspace, a.workspace_bytes = buf.data_ptr(), need - 1
        else:
            a.workspace, a.workspace_bytes = buf.data_ptr() + 8, need
        rc = self._lib.usp_flash_bwd(aref, stream)
        torch.cuda.current_stream().synchronize()          # (buf lives until the launch is done)
        return rc


@contextlib.contextmanager
def _workspace(mode, dev):
    from yunchang_amd import _C
    real = _C.load
    proxy = _WorkspaceProxy(real(), mode, dev)
    _C.load = lambda: proxy
    try:
        yield proxy
    finally:
        _C.load = real


@pytest.mark.parametrize("family", ["row64", "wave32"])
def test_dkdv_heads_sweep_and_workspace_contract(dev, family):
    from yunchang_amd import _C
    case, cus = SWEEP, _cus(dev)
    r = _reference(case, dev)
    scale, G = case.D ** -0.5, case.Hq // case.Hkv
    qs, ks = tuple(r["q"].shape), tuple(r["k"].shape)
    tq, tk, tv, tdo = (r[n] for n in ("q", "k", "v", "do"))
    lse_t, delta_t = r["rl"].float().contiguous(), r["delta"].float().contiguous()
    fam = ("dkdv_row64", "dq_row64") if family == "row64" else ("dkdv_wave8", "dq_wave8")

    def run(heads, expect=None):
        dq, dk, dv = (torch.full(s, float("nan"), dtype=tq.dtype, device=dev) for s in (qs, ks, ks))
        _C.flash_bwd(tdo, tq, tk, tv, lse_t, delta_t, None, None, None, scale, True, dq16=dq, dk16=dk, dv16=dv,
                     family=family, splits=(0, 0), dkdv_heads=heads)
        return (dq, dk, dv), _C.last_launch_kinds()

    assert _bwd_workspace_bytes(case, 0, (0, 0)) == _expected_ws(case, 2, 0, 0), "automatic dkdv_heads != 2 here"
    res = {}
    for heads in (0, 1, 2, 4, 8):
        gsub = heads or 2
        n_items = case.B * case.Hkv * (case.Sk // 128) * (G // gsub)
        assert n_items > cus, (heads, n_items)
        assert _bwd_workspace_bytes(case, heads, (0, 0)) == _expected_ws(case, gsub, 0, 0), heads
        grads, kinds = run(heads)
        assert set(kinds) == set(fam) | ({"reduce_heads"} if gsub < G else set()), (family, heads, kinds)
        _check_bwd(f"{family} dkdv_heads={heads}", grads, r["grads"], case)
        res[heads] = grads
    assert all(_same_bits(a, b) for a, b in zip(res[0], res[2])), "dkdv_heads 0 (auto = 2) and 2 differ"
    for mode in ("none", "short", "misaligned"):
        with _workspace(mode, dev) as proxy:
            grads, kinds = run(2)
        assert proxy.need == _expected_ws(case, 2, 0, 0), (mode, proxy.need)
        assert set(kinds) == set(fam), (family, mode, kinds)
        assert all(_same_bits(a, b) for a, b in zip(grads, res[8])), \
            f"{family}: dkdv_heads=2 with workspace '{mode}' must equal dkdv_heads=8 bit for bit"
    for bad in (3, 16, -1):
        dq, dk, dv = (torch.full(s, float("nan"), dtype=tq.dtype, device=dev) for s in (qs, ks, ks))
        with pytest.raises(RuntimeError):
            _C.flash_bwd(tdo, tq, tk, tv, lse_t, delta_t, None, None, None, scale, True, dq16=dq, dk16=dk, dv16=dv,
                         family=family, splits=(0, 0), dkdv_heads=bad)
        assert _C.last_launch_kinds() == (), (bad, _C.last_launch_kinds())
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (dq, dk, dv)), f"dkdv_heads={bad}: an output was written"


@pytest.mark.parametrize("family", ["row64", "wave32"])
def test_dkdv_heads_must_divide_one_for_mha(dev, family):
    """usp_hip.h: dkdv_heads must divide Hq / Hkv, else USP_EINVAL -- MHA (Hq / Hkv = 1) included: 2 raises before any
    launch and leaves the outputs NaN, 1 runs exactly what 0 runs."""
    from yunchang_amd import _C
    B, S, H, D = 1, 1024, 4, 128
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    q, k, v, do = (torch.randn((B, S, H, D), generator=gen, device=dev).bfloat16() for _ in range(4))
    lse = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    out = torch.empty_like(q)
    _C.flash_fwd(q, k, v, D ** -0.5, True, lse, out=out)
    delta = torch.empty_like(lse)
    _C.bwd_delta(do, out, delta)
    res = {}
    for heads in (0, 1, 2):
        dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
        call = lambda: _C.flash_bwd(do, q, k, v, lse, delta, None, None, None, D ** -0.5, True, dq16=dq, dk16=dk, dv16=dv,
                                    family=family, dkdv_heads=heads)
        if heads == 2:
            with pytest.raises(RuntimeError, match="invalid"):
                call()
            assert _C.last_launch_kinds() == ()
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(t).all()) for t in (dq, dk, dv)), "dkdv_heads=2 (MHA): an output was written"
        else:
            call()
            assert "reduce_heads" not in _C.last_launch_kinds()
            res[heads] = (dq, dk, dv)
    assert all(_same_bits(a, b) for a, b in zip(res[0], res[1]))
    assert all(bool(torch.isfinite(t).all()) for t in res[1])


# ---------------------------------------------------------------------------------------------------------------------
# the ring-step contract at A's shape (c = 4096 rows per half)
# ---------------------------------------------------------------------------------------------------------------------
def test_ring_step_contract_at_rank_block_size(dev):
    """Zigzag-ring steps at the size one rank of the 2 x 4 grid runs: step 0 causal over [0, 2c) into fp32; a later step of
    q[c:] against 2c other keys merges in and finalises rows [c, 2c) in 16 bits; the block backward accumulates onto running
    fp32 gradients with the 16-bit final outputs; and the split backward (only="dq", then only="dkdv") equals the combined
    call bit for bit."""
    from yunchang_amd import _C
    c, B, Hq, Hkv, D = 4096, 1, 16, 2, 128
    dt, scale = "bfloat16", D ** -0.5
    gen = torch.Generator(device=dev)
    gen.manual_seed(41)
    rn = lambda *s: torch.randn(s, generator=gen, device=dev).bfloat16()
    q, do = rn(B, 2 * c, Hq, D), rn(B, 2 * c, Hq, D)
    k1, v1, k2, v2 = (rn(B, 2 * c, Hkv, D) for _ in range(4))
    # exact: rows [0, c) over block 1 (causal); rows [c, 2c) over block 1 (causal) and block 2 (all of it): with block 2's
    # keys put first, bottom-right causal alignment of c rows against 4c keys gives exactly that mask
    ro0, rl0 = ref_fwd(q[:, :c], k1[:, :c], v1[:, :c], scale, True)
    ro1, rl1 = ref_fwd(q[:, c:], torch.cat([k2, k1], 1), torch.cat([v2, v1], 1), scale, True)
    acc = torch.full((B, 2 * c, Hq, D), float("nan"), dtype=torch.float32, device=dev)
    lse = torch.full((B, Hq, 2 * c), float("nan"), dtype=torch.float32, device=dev)
    out = torch.full((B, 2 * c, Hq, D), float("nan"), dtype=q.dtype, device=dev)
    _C.flash_fwd(q, k1, v1, scale, True, lse, out=None, acc=acc, final_begin=0, final_end=0)
    assert B * Hq * (2 * c // 256) > _cus(dev), "step 0 is a multi-pass launch"
    acc0 = acc.clone()
    _C.flash_fwd(q[:, c:], k2, v2, scale, False, lse[:, :, c:], out=out[:, c:], acc=acc[:, c:], merge_in=True,
                 final_begin=0, final_end=c)
    assert_close(out[:, c:], ro1, *TOL[dt]["out"], "ring step: final rows [c, 2c) over both blocks")
    assert_close(lse[:, :, c:], rl1, 2e-3, 1e-4, "ring step: merged lse")
    # (the fp32 rows carry the kernel's 16-bit P products like the 16-bit rows: the stated out tolerance)
    assert_close(acc[:, :c], ro0, *TOL[dt]["out"], "ring step: running rows [0, c) in fp32")
    assert_close(lse[:, :, :c], rl0, 2e-3, 1e-4, "ring step: lse of the running rows")
    assert bool(torch.isnan(out[:, :c]).all()), "ring step: out[:, :c] must not be written"
    assert _same_bits(acc, acc0), "ring step: step 1 must not rewrite the accumulator (its rows are all final)"
    # ---- block backward of step 1 (q[c:] x block 2) with the global lse / delta, onto running fp32 gradients -----------
    o16 = ro1.to(q.dtype)
    qb, dob = q[:, c:].contiguous(), do[:, c:].contiguous()
    lse_g = rl1.float().contiguous()
    delta_g = ref_delta(dob, o16).float().contiguous()
    rdq, rdk, rdv, _ = ref_bwd(dob, qb, k2, v2, o16, rl1, scale, False)
    run_dq, run_dk, run_dv = (torch.randn(s, generator=gen, device=dev) for s in ((B, c, Hq, D), (B, 2 * c, Hkv, D),
                                                                                   (B, 2 * c, Hkv, D)))
    keep = [t.clone() for t in (run_dq, run_dk, run_dv)]
    dq16, dk16, dv16 = (torch.full(t.shape, float("nan"), dtype=q.dtype, device=dev) for t in (run_dq, run_dk, run_dv))
    _C.flash_bwd(dob, qb, k2, v2, lse_g, delta_g, run_dq, run_dk, run_dv, scale, False, accum_dq=True, accum_dk=True,
                 accum_dv=True, dq16=dq16, dk16=dk16, dv16=dv16)
    for got, run, ref, n_ in zip((dq16, dk16, dv16), keep, (rdq, rdk, rdv), ("dq", "dk", "dv")):
        atol, rtol = TOL[dt]["grad"]
        atol = long_sum_atol(atol, 2 * c if n_ == "dq" else c * (Hq // Hkv), ref)
        assert_close(got, run.double() + ref, atol, rtol, f"ring backward: {n_}16 = round(running + block)")
    for t, k_, n_ in zip((run_dq, run_dk, run_dv), keep, ("dq", "dk", "dv")):
        assert _same_bits(t, k_), f"ring backward: the running fp32 {n_} must be left unchanged"
    # ---- split backward: only="dq" then only="dkdv" == the combined call, bit for bit ----------------------------------
    def outs():
        return [torch.full(s, float("nan"), dtype=q.dtype, device=dev) for s in (qb.shape, k2.shape, k2.shape)]
    full, part = outs(), outs()
    _C.flash_bwd(dob, qb, k2, v2, lse_g, delta_g, None, None, None, scale, False, dq16=full[0], dk16=full[1], dv16=full[2])
    kinds_full = set(_C.last_launch_kinds())
    _C.flash_bwd(dob, qb, k2, v2, lse_g, delta_g, None, None, None, scale, False, dq16=part[0], dk16=part[1], dv16=part[2],
                 only="dq")
    kinds_dq = set(_C.last_launch_kinds())
    torch.cuda.synchronize()
    assert bool(torch.isnan(part[1]).all() and torch.isnan(part[2]).all()), "only='dq' wrote dk / dv"
    assert not any(k_.startswith("dkdv") or k_ == "reduce_heads" for k_ in kinds_dq), kinds_dq
    mark = part[0].clone()
    _C.flash_bwd(dob, qb, k2, v2, lse_g, delta_g, None, None, None, scale, False, dq16=part[0], dk16=part[1], dv16=part[2],
                 only="dkdv")
    kinds_kv = set(_C.last_launch_kinds())
    assert not any(k_.startswith("dq") or k_ == "reduce_cuts" for k_ in kinds_kv), kinds_kv
    assert kinds_dq | kinds_kv == kinds_full, (kinds_dq, kinds_kv, kinds_full)
    assert _same_bits(part[0], mark), "only='dkdv' changed dq"
    assert all(_same_bits(a, b) for a, b in zip(part, full)), "split backward != combined backward"
    ring = Case("ring", B, c, 2 * c, Hq, Hkv, D, False, dt, (), (), 4)
    _check_bwd("split backward", full, (rdq, rdk, rdv), ring)


# ---------------------------------------------------------------------------------------------------------------------
# packed batches at size: the dynamic item queue over several passes
# ---------------------------------------------------------------------------------------------------------------------
def test_packed_batch_at_size(dev):
    from yunchang_amd import _C
    lens = (7000, 64, 3000, 1, 5200, 2600, 4100)
    Hq, Hkv, D, dt = 16, 2, 128, "bfloat16"
    scale, T = D ** -0.5, sum(lens)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    rn = lambda *s: torch.randn(s, generator=gen, device=dev).bfloat16()
    q, k, v, do = rn(T, Hq, D), rn(T, Hkv, D), rn(T, Hkv, D), rn(T, Hq, D)
    cu = np.concatenate([[0], np.cumsum(lens)])
    tab = torch.tensor(np.stack([cu[:-1], lens], 1), dtype=torch.int32, device=dev)
    ro = torch.zeros((T, Hq, D), dtype=torch.float64, device=dev)
    rl = torch.zeros((Hq, T), dtype=torch.float64, device=dev)
    for a, b in zip(cu[:-1], cu[1:]):
        o_, l_ = ref_fwd(q[None, a:b], k[None, a:b], v[None, a:b], scale, True)
        ro[a:b], rl[:, a:b] = o_[0], l_[0]
    o16 = ro.to(q.dtype)
    rdq = torch.zeros_like(ro)
    rdk = torch.zeros((T, Hkv, D), dtype=torch.float64, device=dev)
    rdv = torch.zeros_like(rdk)
    for a, b in zip(cu[:-1], cu[1:]):
        g_ = ref_bwd(do[None, a:b], q[None, a:b], k[None, a:b], v[None, a:b], o16[None, a:b], rl[None, :, a:b], scale, True)
        rdq[a:b], rdk[a:b], rdv[a:b] = g_[0][0], g_[1][0], g_[2][0]
    runs = []
    for _ in range(2):
        out = torch.full((T, Hq, D), float("nan"), dtype=q.dtype, device=dev)
        lse = torch.full((Hq, T), float("nan"), dtype=torch.float32, device=dev)
        _C.flash_fwd_packed(q, k, v, tab, tab, max(lens), max(lens), scale, True, lse, out=out)
        runs.append((out, lse))
    assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1]), "packed forward: two runs differ"
    for a, b, n in zip(cu[:-1], cu[1:], lens):
        assert_close(runs[0][0][a:b], ro[a:b], *TOL[dt]["out"], f"packed out, sequence of {n}")
        assert_close(runs[0][1][:, a:b], rl[:, a:b], 2e-3, 1e-4, f"packed lse, sequence of {n}")
    lse_t = rl.float().contiguous()
    delta = ref_delta(do[None], o16[None])[0].float().contiguous()
    grads = []
    for _ in range(2):
        dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
        _C.flash_bwd_packed(do, q, k, v, lse_t, delta, tab, tab, max(lens), max(lens), None, None, None, scale, True,
                            dq16=dq, dk16=dk, dv16=dv)
        grads.append((dq, dk, dv))
    assert all(_same_bits(a_, b_) for a_, b_ in zip(*grads)), "packed backward: two runs differ"
    for a, b, n in zip(cu[:-1], cu[1:], lens):
        for g_, r_, n_ in zip(grads[0], (rdq, rdk, rdv), ("dq", "dk", "dv")):
            atol, rtol = TOL[dt]["grad"]
            atol = long_sum_atol(atol, n if n_ == "dq" else n * (Hq // Hkv), r_[a:b])
            assert_close(g_[a:b], r_[a:b], atol, rtol, f"packed {n_}, sequence of {n}")
    assert int(_C.sched_block(dev).abs().sum()) == 0, "the work-queue control block must be left zeroed"


# ---------------------------------------------------------------------------------------------------------------------
# 64-bit offsets: batch 1 of every 16-bit tensor starts more than 2^32 bytes after batch 0
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["row64", "wave32"])
def test_batch_offsets_beyond_4GiB(dev, family):
    from yunchang_amd import _C
    B, S, Hq, Hkv, D, dt = 2, 2048, 8, 2, 128, "bfloat16"
    scale = D ** -0.5
    sizes = {"q": Hq, "k": Hkv, "v": Hkv, "do": Hq, "out": Hq, "dq": Hq, "dk": Hkv, "dv": Hkv}
    gap = 4096                                             # NaN elements between two views of one batch
    offs, cur = {}, gap
    for n, h in sizes.items():
        offs[n] = cur
        cur += S * h * D + gap
    sb = (1 << 31) + 8192                                  # batch stride in elements: 2^32 + 16 KiB bytes
    assert sb * 2 > (1 << 32) and cur < sb
    arena = torch.full((sb + cur,), float("nan"), dtype=torch.bfloat16, device=dev)
    views = {n: torch.as_strided(arena, (B, S, h, D), (sb, h * D, D, 1), offs[n]) for n, h in sizes.items()}
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    for n in ("q", "k", "v", "do"):
        views[n].copy_(torch.randn(views[n].shape, generator=gen, device=dev).bfloat16())
    q, k, v, do = (views[n] for n in ("q", "k", "v", "do"))
    ro, rl = ref_fwd(q, k, v, scale, True)
    lse = torch.full((B, Hq, S), float("nan"), dtype=torch.float32, device=dev)
    _C.flash_fwd(q, k, v, scale, True, lse, out=views["out"], family=family, k_splits=0)
    # (32 256-row items: the 32-rows-per-wave family takes its 128-row shape)
    assert set(_C.last_launch_kinds()) == ({"fwd_row64"} if family == "row64" else {"fwd_wave4"}), _C.last_launch_kinds()
    _check_fwd(f"offsets > 4 GiB {family}", views["out"], lse, ro, rl, dt)
    o16 = ro.to(q.dtype)
    rdq, rdk, rdv, delta = ref_bwd(do, q, k, v, o16, rl, scale, True)
    _C.flash_bwd(do, q, k, v, rl.float().contiguous(), delta.float().contiguous(), None, None, None, scale, True,
                 dq16=views["dq"], dk16=views["dk"], dv16=views["dv"], family=family, splits=(0, 0), dkdv_heads=1)
    fam = {"dkdv_row64", "dq_row64"} if family == "row64" else {"dkdv_wave8", "dq_wave8"}
    assert set(_C.last_launch_kinds()) == fam | {"reduce_heads"}, _C.last_launch_kinds()
    case = Case("offsets", B, S, S, Hq, Hkv, D, True, dt, (), (), 1)
    _check_bwd(f"offsets > 4 GiB {family}", (views["dq"], views["dk"], views["dv"]), (rdq, rdk, rdv), case)
    spans = sorted((b * sb + offs[n], b * sb + offs[n] + S * h * D) for n, h in sizes.items() for b in range(B))
    edges = [0] + [e for span in spans for e in span] + [arena.numel()]
    for a0, a1 in zip(edges[0::2], edges[1::2]):                # the complement of the views, slice by slice
        assert bool(torch.isnan(arena[a0:a1]).all()), f"a launch wrote between the views (elements [{a0}, {a1}))"
