"""Dropout (dropout_p) on the GPU: the dropout instantiations of the two-waves-per-SIMD kernels (usp_flash_fwd_dropout /
usp_flash_bwd_dropout) against tests/dropout_ref.py (fp64 on the device, the mask from its own numpy Philox), alone and composed
with everything else an argument block says; more work items than CUs; p = 0 through the new entry points; the declines;
hip_attn_func; and LongContextAttention's basic ring on virtual ranks against ONE single-device call with the same seed.

Tolerances: golden_util.TOL / grad_tol with atol multiplied by 256/t -- every surviving rounded product is scaled by that factor
-- rtol unchanged; `lse` (that of the un-dropped scores) takes the plain tolerance.  What a wrong mask costs against these
tolerances is computed without a GPU in tests/test_dropout_cpu.py::test_mutant_references_are_far_away.  Every comparison prints
its largest error as a fraction of its tolerance ([dropout-err] lines; profiles/dropout_rates.txt quotes them).

What these tolerances cannot see: a few wrong mask bits -- a ragged edge, one DPP quad, one patch at a cut -- cost 0.05 to 0.9 of the
backward tolerances and sit within 10 % of the forward's either way (dropout: the table of mutants); 256/t scales the
tolerance, which blinds it at t = 1, and at t = 255 almost nothing differs.  Those are seen in tests/test_gpu_dropout_readout.py,
which makes the kernels print their mask (tests/mask_readout.py) and compares every (batch, head, row, key) bit for bit."""
import os

import pytest
import torch

import dropout_ref
from golden_util import TOL, assert_close, close_mask, grad_tol

pytestmark = pytest.mark.gpu

B, HQ, HKV = 2, 4, 2
SEED = (1 << 40) + 1234                    # above 2^32: both key words matter
FAR = ((1 << 20) + 4, 8, 5)                # (row0, key0, head0) of a block deep inside a long sequence


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _case(dev, Bc, Sq, Sk, Hq, Hkv, D, dt, seed=0):
    g = torch.Generator().manual_seed(seed)
    dtype = getattr(torch, dt)
    return [torch.randn(Bc, s, h, D, generator=g).to(dtype).to(dev) for s, h in ((Sq, Hq), (Sk, Hkv), (Sk, Hkv), (Sq, Hq))]


_IN = {}


def _inputs(dev, Sq, Sk, D, dt):
    key = (Sq, Sk, D, dt)
    if key not in _IN:
        _IN[key] = _case(dev, B, Sq, Sk, HQ, HKV, D, dt, seed=Sq + D)
    return _IN[key]


def _tol(dt, p, what):
    """(atol, rtol): atol x 256/t for out and the gradients, the plain tolerance for the LSE."""
    atol, rtol = TOL[dt]["out"] if what in ("out", "lse") else grad_tol(dt, HQ // HKV)
    return (atol, rtol) if what == "lse" else (atol * dropout_ref.rescale(p), rtol)


def _close(got, want, dt, p, name, what):
    atol, rtol = _tol(dt, p, name)
    _, err = close_mask(got, want, atol, rtol)
    frac = float((err / (atol + rtol * want.abs().to(err.dtype))).nan_to_num(0.0).max())
    print(f"[dropout-err] {what} {name}: {frac:.3f} of tolerance")
    assert_close(got, want, atol, rtol, f"{what} {name}")


def _run_fwd(q, k, v, scale, causal, dropout, **kw):
    from yunchang_amd import _C
    out = torch.full_like(q, float("nan"))
    lse = torch.full((q.shape[0], q.shape[2], q.shape[1]), float("nan"), dtype=torch.float32, device=q.device)
    _C.flash_fwd(q, k, v, scale, causal, lse, out=out, dropout=dropout, **kw)
    return out, lse, _C.last_launch_kinds()


def _run_bwd(do, q, k, v, ref, scale, causal, dropout, **kw):
    from yunchang_amd import _C
    lse = ref[1].to(torch.float32)
    delta = torch.empty_like(lse)
    _C.bwd_delta(do, ref[0].to(q.dtype), delta)
    dq, dk, dv = (torch.full(t.shape, float("nan"), dtype=torch.float32, device=q.device) for t in (q, k, v))
    _C.flash_bwd(do, q, k, v, lse, delta, dq, dk, dv, scale, causal, dropout=dropout, **kw)
    return (dq, dk, dv), _C.last_launch_kinds()


def _check(out, lse, grads, ref, dt, p, what):
    if out is not None:
        _close(out, ref[0], dt, p, "out", what)
        _close(lse, ref[1], dt, p, "lse", what)
    if grads is not None:
        for g, r, name in zip(grads, ref[2:], ("dq", "dk", "dv")):
            _close(g, r, dt, p, name, what)


_WAVE_FWD = {"fwd_wave8", "fwd_wave4", "fwd_split_merge"}
_WAVE_BWD = {"dkdv_wave8", "dq_wave8", "reduce_heads", "reduce_cuts"}


# ---- 1. block parity ---------------------------------------------------------------------------------------------------------
SHAPES = [(320, 200), (129, 513), (256, 256)]      # > 1 query tile of both workgroup shapes, several 64-key tiles, ragged ends


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Sq,Sk", SHAPES)
def test_block_parity(dev, Sq, Sk, causal, D, dt):
    q, k, v, do = _inputs(dev, Sq, Sk, D, dt)
    scale = D ** -0.5
    for p in (0.1, 0.5, 0.9):
        for at in ((0, 0, 0), FAR):
            ref = dropout_ref.ref_bwd(do, q, k, v, scale, p, SEED, at, causal, out_dtype=q.dtype)
            what = f"D{D} {dt} causal {causal} {Sq}x{Sk} p {p} at {at}"
            drop = (p, SEED) + at
            out, lse, kinds = _run_fwd(q, k, v, scale, causal, drop)
            assert kinds and set(kinds) <= _WAVE_FWD, kinds
            grads, kinds = _run_bwd(do, q, k, v, ref, scale, causal, drop)
            assert {"dkdv_wave8", "dq_wave8"} <= set(kinds) <= _WAVE_BWD, kinds
            _check(out, lse, grads, ref, dt, p, what)


# ---- 2. composition with the rest of the argument block ------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dt", [(128, "bfloat16"), (64, "float16")])
def test_composition(dev, D, dt):
    from yunchang_amd import _C
    S, p, at = 512, 0.5, FAR
    q, k, v, do = _inputs(dev, S, S, D, dt)
    scale, drop = D ** -0.5, (p, SEED) + FAR
    for causal in (True, False):
        ref = dropout_ref.ref_bwd(do, q, k, v, scale, p, SEED, at, causal, out_dtype=q.dtype)
        what = f"D{D} {dt} causal {causal}"
        out, lse, kinds = _run_fwd(q, k, v, scale, causal, drop, k_splits=3)
        assert "fwd_split_merge" in kinds and set(kinds) <= _WAVE_FWD, kinds
        _check(out, lse, None, ref, dt, p, f"{what} k_splits 3")
        out, lse, kinds = _run_fwd(q, k, v, scale, causal, drop, interleave=True)
        _check(out, lse, None, ref, dt, p, f"{what} interleave")
        for heads in (1, 2):
            grads, kinds = _run_bwd(do, q, k, v, ref, scale, causal, drop, splits=(2, 2), dkdv_heads=heads)
            assert {"dkdv_wave8", "dq_wave8", "reduce_heads", "reduce_cuts"} == set(kinds), kinds
            _check(None, None, grads, ref, dt, p, f"{what} cuts (2, 2) heads {heads}")
        grads, _ = _run_bwd(do, q, k, v, ref, scale, causal, drop, interleave=True, dkdv_heads=2)
        _check(None, None, grads, ref, dt, p, f"{what} interleave")
        # accum_*: the gradients are added to what the buffers hold
        lse32 = ref[1].to(torch.float32)
        delta = torch.empty_like(lse32)
        _C.bwd_delta(do, ref[0].to(q.dtype), delta)
        base = [torch.full(t.shape, 0.5, dtype=torch.float32, device=dev) for t in (q, k, v)]
        _C.flash_bwd(do, q, k, v, lse32, delta, *base, scale, causal, True, True, True, dropout=drop)
        _check(None, None, [g - 0.5 for g in base], ref, dt, p, f"{what} accum")
        # the 16-bit final outputs
        g16 = [torch.full_like(t, float("nan")) for t in (q, k, v)]
        _C.flash_bwd(do, q, k, v, lse32, delta, None, None, None, scale, causal, dq16=g16[0], dk16=g16[1], dv16=g16[2], dropout=drop)
        _check(None, None, g16, ref, dt, p, f"{what} 16-bit outputs")
    # a window and a shift
    for causal, window, shift in ((True, (64, 0), None), (False, (64, 0), None), (True, None, -96), (False, (100, 40), 64)):
        ref = dropout_ref.ref_bwd(do, q, k, v, scale, p, SEED, at, causal, window, shift or 0, out_dtype=q.dtype)
        kw = dict(window=window, shift=shift)
        out, lse, _ = _run_fwd(q, k, v, scale, causal, drop, **kw)
        grads, _ = _run_bwd(do, q, k, v, ref, scale, causal, drop, **kw)
        _check(out, lse, grads, ref, dt, p, f"D{D} causal {causal} window {window} shift {shift}")
    # merge_in with an acc and a partial final range: two calls forming one ring row; the second block's keys lie `h` further
    ref = dropout_ref.ref_bwd(do, q, k, v, scale, p, SEED, at, False, out_dtype=q.dtype)
    acc = torch.full(q.shape, float("nan"), dtype=torch.float32, device=dev)
    out2 = torch.full_like(q, float("nan"))
    lse2 = torch.full((B, HQ, S), float("nan"), dtype=torch.float32, device=dev)
    h = 192
    _C.flash_fwd(q, k[:, :h], v[:, :h], scale, False, lse2, out=out2, acc=acc, final_end=0, dropout=drop)
    _C.flash_fwd(q, k[:, h:], v[:, h:], scale, False, lse2, out=out2, acc=acc, merge_in=True, final_begin=50, final_end=150,
                 dropout=(p, SEED, at[0], at[1] + h, at[2]))
    _close(lse2, ref[1], dt, p, "lse", "merged")
    _close(out2[:, 50:150], ref[0][:, 50:150], dt, p, "out", "merged, final rows")
    _close(torch.cat([acc[:, :50], acc[:, 150:]], 1), torch.cat([ref[0][:, :50], ref[0][:, 150:]], 1), dt, p, "out",
           "merged, running rows")


# ---- 2b. the 8-wave forward (256-row workgroups): what large shapes get -------------------------------------------------------------
# The library takes 8 waves when B * Hq * ceil(Sq / 256) * k_splits >= 256 and a causal launch has more than 1024 rows
# (usp_flash_fwd.hip: launch_fwd); every B2 H4 case above therefore runs the 4-wave kernel.  B2 H32/8 S1152: 320 items of 256 rows,
# 4.5 query tiles, 18 key tiles.  Forward only: the backward kernels have one workgroup shape.  Inputs lie on a 1/16 grid, exact in
# bf16 and in fp16, so the two dtypes share one fp64 reference per (D, mask); the mask's bytes are generated once for all cases.
W8 = dict(B=2, Hq=32, Hkv=8, S=1152, at=(2048, 4096, 8))
_W8_IN, _W8_REF = {}, {}


def _w8_inputs(dev, D):
    if D not in _W8_IN:
        g = torch.Generator().manual_seed(40 + D)
        _W8_IN[D] = [(torch.randn(W8["B"], W8["S"], h, D, generator=g) * 16).round().clamp(-64, 64).div(16).to(dev)
                     for h in (W8["Hq"], W8["Hkv"], W8["Hkv"])]
    return _W8_IN[D]


def _w8_ref(dev, D, p, causal, window=None):
    key = (D, p, causal, window)
    if key not in _W8_REF:
        q, k, v = _w8_inputs(dev, D)
        _W8_REF[key] = dropout_ref.ref_fwd(q, k, v, D ** -0.5, p, SEED, W8["at"], causal, window)
    return _W8_REF[key]


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D,dt,p", [(128, "bfloat16", 0.1), (128, "float16", 0.5), (32, "float16", 0.1), (64, "bfloat16", 0.9)])
def test_eight_wave_forward(dev, D, dt, p, causal):
    from yunchang_amd import _C
    q, k, v = (t.to(getattr(torch, dt)) for t in _w8_inputs(dev, D))
    assert all(torch.equal(a.float(), b) for a, b in zip((q, k, v), _w8_inputs(dev, D))), "the inputs are exact in both dtypes"
    scale, S, drop = D ** -0.5, W8["S"], (p, SEED) + W8["at"]
    what = f"8 waves D{D} {dt} causal {causal} p {p}"
    ref = _w8_ref(dev, D, p, causal)
    out, lse, kinds = _run_fwd(q, k, v, scale, causal, drop, k_splits=0)
    assert kinds == ("fwd_wave8",), kinds
    _check(out, lse, None, ref, dt, p, what)
    out, lse, kinds = _run_fwd(q, k, v, scale, causal, drop, k_splits=2)
    assert set(kinds) == {"fwd_wave8", "fwd_split_merge"}, kinds
    _check(out, lse, None, ref, dt, p, f"{what} k_splits 2")
    window = (200, 0) if causal else (200, 70)
    refw = _w8_ref(dev, D, p, causal, window)
    out, lse, kinds = _run_fwd(q, k, v, scale, causal, drop, window=window, k_splits=0)
    assert kinds == ("fwd_wave8",), kinds
    _check(out, lse, None, refw, dt, p, f"{what} window {window}")
    if not causal:        # merge_in: two key runs forming one ring row, rows [300, 700) final; the second run's keys lie `h` further
        acc = torch.full(q.shape, float("nan"), dtype=torch.float32, device=dev)
        out2 = torch.full_like(q, float("nan"))
        lse2 = torch.full((W8["B"], W8["Hq"], S), float("nan"), dtype=torch.float32, device=dev)
        h, at = 448, W8["at"]
        _C.flash_fwd(q, k[:, :h], v[:, :h], scale, False, lse2, out=out2, acc=acc, final_end=0, k_splits=0, dropout=drop)
        assert _C.last_launch_kinds() == ("fwd_wave8",)
        _C.flash_fwd(q, k[:, h:], v[:, h:], scale, False, lse2, out=out2, acc=acc, merge_in=True, final_begin=300, final_end=700,
                     k_splits=0, dropout=(p, SEED, at[0], at[1] + h, at[2]))
        assert _C.last_launch_kinds() == ("fwd_wave8",)
        _close(lse2, ref[1], dt, p, "lse", f"{what} merged")
        _close(out2[:, 300:700], ref[0][:, 300:700], dt, p, "out", f"{what} merged, final rows")
        _close(torch.cat([acc[:, :300], acc[:, 700:]], 1), torch.cat([ref[0][:, :300], ref[0][:, 700:]], 1), dt, p, "out",
               f"{what} merged, running rows")


# ---- 3. more work items than CUs in one launch ------------------------------------------------------------------------------------------
def test_more_items_than_cus(dev):
    """A persistent multi-pass walk; the causal launch takes the 4-wave workgroups, the full one the 8-wave ones (asserted): both
    workgroup shapes of the forward."""
    Bc, S, Hq, Hkv, D, dt, p = 5, 512, 32, 8, 64, "bfloat16", 0.5
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    q, k, v, do = _case(dev, Bc, S, S, Hq, Hkv, D, dt, seed=5)
    scale, at = D ** -0.5, (8, 4, 3)
    for causal in (True, False):
        fwd_items = Bc * Hq * ((S + 127) // 128 if causal else (S + 255) // 256)
        assert fwd_items > cus * (2 if causal else 1) and Bc * Hq * ((S + 255) // 256) > cus and Bc * Hkv * ((S + 127) // 128) * 2 > cus
        ref = dropout_ref.ref_bwd(do, q, k, v, scale, p, SEED, at, causal, out_dtype=q.dtype)
        what = f"B{Bc} H{Hq}/{Hkv} S{S} causal {causal}"
        out, lse, kinds = _run_fwd(q, k, v, scale, causal, (p, SEED) + at)
        assert kinds == (("fwd_wave4",) if causal else ("fwd_wave8",)), kinds
        _check(out, lse, None, ref, dt, p, what)
        for heads in (0, 2, 4):
            grads, kinds = _run_bwd(do, q, k, v, ref, scale, causal, (p, SEED) + at, dkdv_heads=heads)
            assert {"dkdv_wave8", "dq_wave8"} <= set(kinds), kinds
            _check(None, None, grads, ref, dt, p, f"{what} heads {heads}")
        del ref


# ---- 4. p = 0 is the plain entry points; the seed decides the mask ---------------------------------------------------------------------
class _ZeroDropout:
    """The loaded library with usp_flash_fwd / usp_flash_bwd routed through the *_dropout entry points with p_drop = 0 (and
    offsets that would be declined with dropout on: they are ignored)."""

    def __init__(self, L, p):
        from yunchang_amd import _C
        self._L, self._p = L, p
        self._f, self._b = _C._dropout_entry("usp_flash_fwd_dropout"), _C._dropout_entry("usp_flash_bwd_dropout")

    def usp_flash_fwd(self, a, stream):
        return self._f(a, self._p, 77, 3, -5, 1, stream)

    def usp_flash_bwd(self, a, stream):
        return self._b(a, self._p, 77, 3, -5, 1, stream)

    def __getattr__(self, name):
        return getattr(self._L, name)


@pytest.mark.parametrize("D,family,p0", [(128, None, 0.0), (128, "wave32", 1.0 / 1024), (64, None, 0.0)])
def test_zero_dropout_is_the_plain_entry_points(dev, monkeypatch, D, family, p0):
    from yunchang_amd import _C
    dt, Sq, Sk = "bfloat16", 320, 200
    q, k, v, do = _inputs(dev, Sq, Sk, D, dt)
    scale = D ** -0.5
    ref = dropout_ref.ref_bwd(do, q, k, v, scale, 0.0, 0, (0, 0, 0), True, out_dtype=q.dtype)
    runs = []
    real = _C.load()
    for lib in (real, _ZeroDropout(real, p0)):       # (p0 = 1/1024: a threshold of 256, also the plain call)
        monkeypatch.setattr(_C, "load", lambda lib=lib: lib)
        out, lse, fk = _run_fwd(q, k, v, scale, True, None, family=family)
        grads, bk = _run_bwd(do, q, k, v, ref, scale, True, None, family=family)
        runs.append(((out, lse) + grads, fk, bk))
    monkeypatch.setattr(_C, "load", lambda: real)
    assert runs[0][1:] == runs[1][1:], (runs[0][1:], runs[1][1:])
    if D == 128 and family is None:
        assert "dkdv_row64" in runs[1][2] and "dq_row64" in runs[1][2], runs[1][2]      # p = 0 keeps the 64-row family
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    # the same seed twice: bit-identical; seed + 1: another mask
    p = 0.5
    rd = dropout_ref.ref_bwd(do, q, k, v, scale, p, SEED, (0, 0, 0), True, out_dtype=q.dtype)
    a = _run_fwd(q, k, v, scale, True, (p, SEED, 0, 0, 0))[:2] + _run_bwd(do, q, k, v, rd, scale, True, (p, SEED, 0, 0, 0))[0]
    b = _run_fwd(q, k, v, scale, True, (p, SEED, 0, 0, 0))[:2] + _run_bwd(do, q, k, v, rd, scale, True, (p, SEED, 0, 0, 0))[0]
    c = _run_fwd(q, k, v, scale, True, (p, SEED + 1, 0, 0, 0))[:2] + _run_bwd(do, q, k, v, rd, scale, True, (p, SEED + 1, 0, 0, 0))[0]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(a[1], c[1]), "the LSE does not see the mask"
    assert all(not torch.equal(x, y) for x, y in zip(a[:1] + a[2:], c[:1] + c[2:]))


# ---- 5. the declines, on the device: nothing is written ---------------------------------------------------------------------------------
def test_declines_on_the_device(dev):
    from yunchang_amd import _C
    D, dt = 128, "bfloat16"
    q, k, v, do = _inputs(dev, 320, 200, D, dt)
    scale = D ** -0.5
    ok = (0.5, SEED, 0, 0, 0)
    cases = [(dict(softcap=30.0), ok, -2), (dict(family="row64"), ok, -2), ({}, (0.5, SEED, 2, 0, 0), -2), ({}, (0.5, SEED, 0, 6, 0), -2),
             ({}, (0.5, SEED, (1 << 31) - 320, 0, 0), -2), ({}, (0.5, SEED, 0, (1 << 31) - 200, 0), -2)]
    for kw, drop, code in cases:
        out = torch.full_like(q, 7.0)
        lse = torch.full((B, HQ, 320), 7.0, dtype=torch.float32, device=dev)
        with pytest.raises(RuntimeError, match=f"code {code}"):
            _C.flash_fwd(q, k, v, scale, True, lse, out=out, dropout=drop, **kw)
        assert _C.last_launch_kinds() == () and bool((out == 7.0).all()) and bool((lse == 7.0).all()), (kw, drop)
        stat = torch.zeros(B, HQ, 320, dtype=torch.float32, device=dev)
        grads = [torch.full(t.shape, 7.0, dtype=torch.float32, device=dev) for t in (q, k, v)]
        with pytest.raises(RuntimeError, match=f"code {code}"):
            _C.flash_bwd(do, q, k, v, stat, stat, *grads, scale, True, dropout=drop, **kw)
        assert _C.last_launch_kinds() == () and all(bool((g == 7.0).all()) for g in grads), (kw, drop)
    for bad in ((float("nan"), 1, 0, 0, 0), (-0.1, 1, 0, 0, 0), (1.0, 1, 0, 0, 0), (0.5, 1, -4, 0, 0), (0.5, -1, 0, 0, 0)):
        with pytest.raises(ValueError):
            _run_fwd(q, k, v, scale, True, bad)
    with pytest.raises(NotImplementedError, match="alibi"):
        _run_fwd(q, k, v, scale, True, ok, alibi=torch.ones(HQ, dtype=torch.float32, device=dev))
    # unforced D = 128 runs on the two-waves-per-SIMD family
    ref = dropout_ref.ref_bwd(do, q, k, v, scale, 0.5, SEED, (0, 0, 0), True, out_dtype=q.dtype)
    _, _, kinds = _run_fwd(q, k, v, scale, True, ok)
    assert kinds in (("fwd_wave8",), ("fwd_wave4",)), kinds
    _, kinds = _run_bwd(do, q, k, v, ref, scale, True, ok)
    assert "dkdv_wave8" in kinds and "dq_wave8" in kinds and not any("row64" in x for x in kinds), kinds


# ---- 6. the Python entry points -------------------------------------------------------------------------------------------------------
def test_hip_attn_func_autograd_at_a_padded_head_dim(dev):
    from yunchang_amd.kernels.attention import draw_seed, hip_attn_backward, hip_attn_forward, hip_attn_func
    D, dt, p = 96, "bfloat16", 0.1
    q, k, v, do = _case(dev, B, 320, 200, HQ, HKV, D, dt, seed=9)
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    torch.manual_seed(77)
    out, lse, none = hip_attn_func(*leaves, dropout_p=p, causal=True, return_attn_probs=True)
    assert none is None
    out.backward(do)
    torch.manual_seed(77)
    seed = draw_seed()                                   # the seed the call drew
    ref = dropout_ref.ref_bwd(do, q, k, v, D ** -0.5, p, seed, (0, 0, 0), True, out_dtype=q.dtype)
    _close(out, ref[0], dt, p, "out", "hip_attn_func")
    _close(lse, ref[1], dt, p, "lse", "hip_attn_func")
    for t, r, name in zip(leaves, ref[2:], ("dq", "dk", "dv")):
        _close(t.grad, r, dt, p, name, "hip_attn_func")
    o2, l2 = hip_attn_forward(q, k, v, dropout_p=p, causal=True, rng_state=seed)
    assert torch.equal(o2, out.detach()) and torch.equal(l2, lse)
    g = [torch.full_like(t, float("nan")) for t in (q, k, v)]
    hip_attn_backward(do, q, k, v, o2, l2, *g, dropout_p=p, bwd_causal=True, rng_state=(seed, 0, 0, 0))
    for a, t, name in zip(g, leaves, ("dq", "dk", "dv")):
        assert torch.equal(a, t.grad), name
    with pytest.raises(NotImplementedError, match="rng_state"):
        hip_attn_forward(q, k, v, dropout_p=p, causal=True)


# ---- 7. grid invariance on virtual ranks ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nccl_single():
    import torch.distributed as dist
    import yunchang_amd  # noqa: F401
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29739")
    own = not dist.is_initialized()
    if own:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    yield dist
    if own:
        dist.destroy_process_group()


def _virtual_run(monkeypatch, nccl_single, dev, ud, rd, rows, causal, p, seed):
    """Every rank of a ud x rd grid as a thread: the Ulysses exchange by hand (autograd cannot run the ranks' backwards side by
    side), then the basic ring's forward and backward of the package with the real HipBlockBackend, the state (seed, head0) as
    the layer and the ring front end hand it down: head0 = local_heads(H, P, rank).start.  Returns per rank (out, dq, dk, dv)
    and the unsharded inputs."""
    import yunchang_amd.comm.all_to_all as A
    import yunchang_amd.ring.ring_flash_attn as R
    from yunchang_amd.kernels import get_block_backend
    from virtual_grid import VirtualGridPairwise, patch_dist, run_grid
    assert get_block_backend().name == "hip"
    grid = VirtualGridPairwise(ud, rd, nccl_single)
    patch_dist(monkeypatch, grid)
    ws, D = ud * rd, 64
    S = rows * ws
    q, k, v, do = _case(dev, 1, S, S, HQ, HKV, D, "bfloat16", seed=4)
    loc = [[t[:, r * rows:(r + 1) * rows].contiguous() for t in (q, k, v, do)] for r in range(ws)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(ws)]
    scale = D ** -0.5
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        upg, rpg = grid.groups_of(r)
        lq, lk, lv, ldo = loc[r]
        kw = dict(causal=causal, dropout_p=p, rng_state=(seed, A.local_heads(HQ, ud, r % ud).start))
        with torch.cuda.stream(streams[r]):
            hq, hdo = (A.heads_to_seq(t, upg, contiguous=True) for t in (lq, ldo))
            hk, hv = (A.kv_heads_to_seq(t, upg, contiguous=True) for t in (lk, lv))
            out, lse = R.ring_flash_attn_forward(rpg, hq, hk, hv, scale, **kw)
            dq, dk, dv = R.ring_flash_attn_backward(rpg, hdo, hq, hk, hv, out, lse, scale, **kw)
            return [A.seq_to_heads(out, upg), A.seq_to_heads(dq, upg), A.kv_seq_to_heads(dk, upg, HKV), A.kv_seq_to_heads(dv, upg, HKV)]
    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    return res, (q, k, v, do)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("ud,rd", [(1, 2), (2, 2), (1, 4)])
def test_grid_invariance_on_virtual_ranks(dev, nccl_single, monkeypatch, ud, rd, causal):
    """Every rank's out, dq, dk, dv against ONE single-device hip_attn_func call on the unsharded tensors with the same seed."""
    from yunchang_amd.kernels.attention import draw_seed, hip_attn_func
    rows, p, dt = 128, 0.5, "bfloat16"
    torch.manual_seed(5)
    seed = draw_seed()
    res, (q, k, v, do) = _virtual_run(monkeypatch, nccl_single, dev, ud, rd, rows, causal, p, seed)
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    torch.manual_seed(5)                                  # hip_attn_func draws the same seed
    one = hip_attn_func(*leaves, dropout_p=p, causal=causal)
    one.backward(do)
    single = (one.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad)
    plain = hip_attn_func(q, k, v, causal=causal)
    assert float((plain.float() - single[0].float()).abs().max()) > 0.5, "dropout changed nothing"
    for r in range(ud * rd):
        sl = slice(r * rows, (r + 1) * rows)
        for got, want, name in zip(res[r], single, ("out", "dq", "dk", "dv")):
            _close(got.float(), want[:, sl].double(), dt, p, name, f"{ud}x{rd} causal {causal} rank {r}")
