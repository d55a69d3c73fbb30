"""ALiBi (alibi_slopes) on the GPU: the ALiBi instantiations of the two-waves-per-SIMD kernels (usp_flash_fwd_alibi /
usp_flash_bwd_alibi) against tests/alibi_ref.py (fp64, on the device), alone and composed with everything else an argument block
says; more work items than CUs (the slope is read per item); NULL slopes; hip_attn_func; the declines; and the basic ring under
USP_RING_ALIBI=global on virtual ranks (real kernels, real RCCL self send/recv).

The base case is B2, Hq4 / Hkv2, (Sq, Sk) = (300, 459) and (459, 300): ragged against the 64-key tile, the 128-key dK/dV block
and the 256-row item, and Sk != Sq makes the diagonal term matter.  Slopes are (B, Hq): batch 0 = default_slopes(4), batch 1 the
same reversed -- a kernel that reads the wrong head's or the wrong batch's slope, drops Sk - Sq or the whole bias is far
outside the tolerance (`test_mutant_references_are_far_away` computes by how much, with the reference alone).  Under `causal` an
off-by-one diagonal cancels in out and in the gradients (a row-constant term) and shows only in the LSE, by the slope: the LSE
is checked in every forward case, at TOL[dt]["out"] like out."""
import ctypes
import os

import pytest
import torch

import alibi_ref
from golden_util import TOL, assert_close, grad_tol

pytestmark = pytest.mark.gpu

B, HQ, HKV = 2, 4, 2


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _case(dev, Bc, Sq, Sk, Hq, Hkv, D, dt, seed=0):
    g = torch.Generator().manual_seed(seed)
    dtype = getattr(torch, dt)
    return [torch.randn(Bc, s, h, D, generator=g).to(dtype).to(dev) for s, h in ((Sq, Hq), (Sk, Hkv), (Sk, Hkv), (Sq, Hq))]


def _slopes(dev, kind="2d", H=HQ):
    m = alibi_ref.default_slopes(H, dev)
    return torch.stack([m, m.flip(0)]) if kind == "2d" else m


_REF, _IN = {}, {}


def _inputs(dev, Sq, Sk, D, dt):
    key = (Sq, Sk, D, dt)
    if key not in _IN:
        _IN[key] = _case(dev, B, Sq, Sk, HQ, HKV, D, dt, seed=Sq + D)
    return _IN[key]


def _reference(key, do, q, k, v, scale, slopes, causal=False, window=None, shift=0):
    """(out, lse, dq, dk, dv) fp64 on the device, computed once per case and shared (never modified)."""
    if key not in _REF:
        _REF[key] = alibi_ref.ref_bwd(do, q, k, v, scale, slopes, causal, window, shift, out_dtype=q.dtype)
    return _REF[key]


def _run_fwd(q, k, v, scale, causal, slopes, **kw):
    from yunchang_amd import _C
    out = torch.full_like(q, float("nan"))
    lse = torch.full((q.shape[0], q.shape[2], q.shape[1]), float("nan"), dtype=torch.float32, device=q.device)
    _C.flash_fwd(q, k, v, scale, causal, lse, out=out, alibi=slopes, **kw)
    return out, lse, _C.last_launch_kinds()


def _run_bwd(do, q, k, v, ref, scale, causal, slopes, **kw):
    from yunchang_amd import _C
    lse = ref[1].to(torch.float32)
    delta = torch.empty_like(lse)
    _C.bwd_delta(do, ref[0].to(q.dtype), delta)
    dq, dk, dv = (torch.full(t.shape, float("nan"), dtype=torch.float32, device=q.device) for t in (q, k, v))
    _C.flash_bwd(do, q, k, v, lse, delta, dq, dk, dv, scale, causal, alibi=slopes, **kw)
    return (dq, dk, dv), _C.last_launch_kinds()


def _check_fwd(out, lse, ref, dt, what):
    assert_close(out, ref[0], *TOL[dt]["out"], f"{what} out")
    assert_close(lse, ref[1], *TOL[dt]["out"], f"{what} lse")


def _check_bwd(grads, ref, dt, what):
    for g, r, name in zip(grads, ref[2:], ("dq", "dk", "dv")):
        assert_close(g, r, *grad_tol(dt, HQ // HKV), f"{what} {name}")


_WAVE_FWD = {"fwd_wave8", "fwd_wave4", "fwd_split_merge"}
_WAVE_BWD = {"dkdv_wave8", "dq_wave8", "reduce_heads", "reduce_cuts"}


# ---- 1. block parity ---------------------------------------------------------------------------------------------------------
PARITY = [(D, dt, causal, sq, sk, "2d") for D in (64, 128) for dt in ("bfloat16", "float16") for causal in (False, True)
          for sq, sk in ((300, 459), (459, 300))] + [(32, "bfloat16", True, 300, 459, "2d"), (32, "float16", False, 459, 300, "2d"),
                                                     (64, "bfloat16", False, 300, 459, "1d"), (128, "float16", True, 300, 459, "1d")]


@pytest.mark.parametrize("D,dt,causal,Sq,Sk,kind", PARITY, ids=lambda v: str(v))
def test_block_parity(dev, D, dt, causal, Sq, Sk, kind):
    q, k, v, do = _inputs(dev, Sq, Sk, D, dt)
    scale, m = D ** -0.5, _slopes(dev, kind)
    ref = _reference(("blk", D, dt, causal, Sq, Sk, kind), do, q, k, v, scale, m, causal)
    what = f"D{D} {dt} causal {causal} {Sq}x{Sk} slopes {kind}"
    out, lse, kinds = _run_fwd(q, k, v, scale, causal, m)
    assert kinds and set(kinds) <= _WAVE_FWD, kinds
    _check_fwd(out, lse, ref, dt, what)
    grads, kinds = _run_bwd(do, q, k, v, ref, scale, causal, m)
    assert {"dkdv_wave8", "dq_wave8"} <= set(kinds) <= _WAVE_BWD, kinds
    _check_bwd(grads, ref, dt, what)


# ---- 2. what the tolerances can see, computed with the reference alone ---------------------------------------------------------------
def test_mutant_references_are_far_away(dev):
    """Non-causal 300 x 459, D64, bf16 inputs.  Each wrong reference differs from the true one by more than 10 x the bf16 tolerance
    (out 2e-2, gradients 5e-2) in out, dq, dk and dv: no ALiBi, slopes reversed across heads, batch 0's slopes for both batches,
    the Sk - Sq term dropped.  The diagonal off by one: more than 5 x.  Under `causal` an off-by-one diagonal is a row-constant
    term: invisible in out and the gradients, and in the LSE exactly the slope (0.25 for head 0 of batch 0)."""
    D, dt = 64, "bfloat16"
    Sq, Sk = 300, 459
    q, k, v, do = _inputs(dev, Sq, Sk, D, dt)
    scale, m = D ** -0.5, _slopes(dev)
    true = _reference(("blk", D, dt, False, Sq, Sk, "2d"), do, q, k, v, scale, m, False)
    names = ("out", "lse", "dq", "dk", "dv")
    atol = dict(out=TOL[dt]["out"][0], dq=grad_tol(dt)[0], dk=grad_tol(dt)[0], dv=grad_tol(dt)[0])

    def gaps(wrong):
        return {n: float((a - b).abs().max()) for n, a, b in zip(names, true, wrong) if n != "lse"}
    mutants = {"no alibi": alibi_ref.ref_bwd(do, q, k, v, scale, None, out_dtype=q.dtype),
               "heads reversed": alibi_ref.ref_bwd(do, q, k, v, scale, m.flip(1), out_dtype=q.dtype),
               "batch 0 for both": alibi_ref.ref_bwd(do, q, k, v, scale, m[0], out_dtype=q.dtype),
               "Sk - Sq dropped": alibi_ref.ref_bwd(do, q, k, v, scale, m, shift=-(Sk - Sq), out_dtype=q.dtype)}
    for name, wrong in mutants.items():
        g = gaps(wrong)
        print(f"[alibi-mutant] {name}: " + " ".join(f"{n}={x:.3f}" for n, x in g.items()))
        assert all(g[n] > 10 * atol[n] for n in g), (name, g)
    g = gaps(alibi_ref.ref_bwd(do, q, k, v, scale, m, shift=1, out_dtype=q.dtype))
    print("[alibi-mutant] diagonal + 1: " + " ".join(f"{n}={x:.3f}" for n, x in g.items()))
    assert all(g[n] > 5 * atol[n] for n in g), g
    c0 = alibi_ref.ref_fwd(q, k, v, scale, m, causal=True)
    # (the mask stays where it is: only the bias diagonal moves -- the bias of row i is then m (i + off + 1 - j) = bias + m)
    s1 = alibi_ref._scores(q, k, scale, m, True, None, 0)[0] - m.double()[:, :, None, None]
    l1 = torch.logsumexp(s1, -1)
    assert float((l1 - c0[1])[0, 0].abs().max()) == pytest.approx(0.25, abs=1e-9)
    o1 = torch.einsum("bhij,bjhd->bihd", alibi_ref._probs(s1, l1), v.double().repeat_interleave(HQ // HKV, dim=2))
    assert float((o1 - c0[0]).abs().max()) < 1e-9


# ---- 3. composition with the rest of the argument block ------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dt", [(128, "bfloat16"), (64, "float16")])
def test_composition(dev, D, dt):
    from yunchang_amd import _C
    Sq, Sk = 300, 459
    q, k, v, do = _inputs(dev, Sq, Sk, D, dt)
    scale, m = D ** -0.5, _slopes(dev)
    # windows
    for window, causal in (((100, 37), False), ((100, 0), True)):
        ref = _reference(("win", D, dt, window), do, q, k, v, scale, m, causal, window)
        out, lse, _ = _run_fwd(q, k, v, scale, causal, m, window=window)
        _check_fwd(out, lse, ref, dt, f"D{D} window {window}")
        grads, _ = _run_bwd(do, q, k, v, ref, scale, causal, m, window=window)
        _check_bwd(grads, ref, dt, f"D{D} window {window}")
    for causal in (False, True):
        ref = _reference(("blk", D, dt, causal, Sq, Sk, "2d"), do, q, k, v, scale, m, causal)
        what = f"D{D} {dt} causal {causal}"
        # K split, interleaved launch
        out, lse, kinds = _run_fwd(q, k, v, scale, causal, m, k_splits=2)
        assert "fwd_split_merge" in kinds and set(kinds) <= _WAVE_FWD, kinds
        _check_fwd(out, lse, ref, dt, f"{what} k_splits 2")
        out, lse, kinds = _run_fwd(q, k, v, scale, causal, m, interleave=True)
        _check_fwd(out, lse, ref, dt, f"{what} interleave")
        # backward cuts with one and two heads per dK/dV item, interleaved, one launch at a time
        for heads in (1, 2):
            grads, kinds = _run_bwd(do, q, k, v, ref, scale, causal, m, splits=(2, 2), dkdv_heads=heads)
            assert {"dkdv_wave8", "dq_wave8", "reduce_heads", "reduce_cuts"} == set(kinds), kinds
            _check_bwd(grads, ref, dt, f"{what} cuts (2, 2) heads {heads}")
        grads, _ = _run_bwd(do, q, k, v, ref, scale, causal, m, interleave=True, dkdv_heads=2)
        _check_bwd(grads, ref, dt, f"{what} interleave")
        (dq, dk, dv), kinds = _run_bwd(do, q, k, v, ref, scale, causal, m, only="dq")
        assert kinds == ("dq_wave8",) and bool(torch.isnan(dk).all()) and bool(torch.isnan(dv).all())
        assert_close(dq, ref[2], *grad_tol(dt), f"{what} only dq")
        (dq, dk, dv), kinds = _run_bwd(do, q, k, v, ref, scale, causal, m, only="dkdv")
        assert "dkdv_wave8" in kinds and "dq_wave8" not in kinds and bool(torch.isnan(dq).all())
        assert_close(dk, ref[3], *grad_tol(dt, 2), f"{what} only dkdv: dk")
        assert_close(dv, ref[4], *grad_tol(dt, 2), f"{what} only dkdv: dv")
    # merge_in with partial final rows: two key runs, the first adopts, the second merges; rows [50, 150) are final
    ref = _reference(("blk", D, dt, False, Sq, Sk, "2d"), do, q, k, v, scale, m, False)
    acc = torch.full(q.shape, float("nan"), dtype=torch.float32, device=dev)
    out2 = torch.full_like(q, float("nan"))
    lse2 = torch.full((B, HQ, Sq), float("nan"), dtype=torch.float32, device=dev)
    h = 192
    _C.flash_fwd(q, k[:, :h], v[:, :h], scale, False, lse2, out=out2, acc=acc, final_end=0, shift=Sk - h, alibi=m)
    _C.flash_fwd(q, k[:, h:], v[:, h:], scale, False, lse2, out=out2, acc=acc, merge_in=True, final_begin=50, final_end=150,
                 shift=0, alibi=m)                     # (bottom-right alignment: the trailing keys keep the diagonal)
    assert_close(lse2, ref[1], *TOL[dt]["out"], "merged lse")
    assert_close(out2[:, 50:150], ref[0][:, 50:150], *TOL[dt]["out"], "merged out, final rows")
    assert_close(torch.cat([acc[:, :50], acc[:, 150:]], 1), torch.cat([ref[0][:, :50], ref[0][:, 150:]], 1), *TOL[dt]["out"],
                 "merged out, running rows")


SHIFTS = [(320, False), (-320, False), (320, True), (-100, True), (-700, True)]      # the last one empties the launch


@pytest.mark.parametrize("D,dt", [(128, "bfloat16"), (64, "float16")])
def test_shifted_diagonal(dev, D, dt):
    """A shift moves the bias with neither `causal` nor a window, and bias and mask together with one."""
    Sq, Sk = 300, 459
    q, k, v, do = _inputs(dev, Sq, Sk, D, dt)
    scale, m = D ** -0.5, _slopes(dev)
    for shift, causal in SHIFTS:
        ref = _reference(("shift", D, dt, shift, causal), do, q, k, v, scale, m, causal, None, shift)
        what = f"D{D} {dt} shift {shift} causal {causal}"
        out, lse, _ = _run_fwd(q, k, v, scale, causal, m, shift=shift)
        _check_fwd(out, lse, ref, dt, what)
        grads, _ = _run_bwd(do, q, k, v, ref, scale, causal, m, shift=shift)
        _check_bwd(grads, ref, dt, what)
        if shift == -700:
            assert bool((out == 0).all()) and bool(torch.isinf(lse).all()) and bool((lse < 0).all())
            assert all(bool((g == 0).all()) for g in grads)
    moved = _reference(("shift", D, dt, 320, False), do, q, k, v, scale, m, False, None, 320)
    plain = _reference(("blk", D, dt, False, Sq, Sk, "2d"), do, q, k, v, scale, m, False)
    assert float((moved[0] - plain[0]).abs().max()) > 10 * TOL[dt]["out"][0], "a shift without a bound is not a no-op with ALiBi"


# ---- 4. more work items than CUs in one launch: the slope is read again for every item of the persistent walk ---------------------
def test_more_items_than_cus(dev):
    from yunchang_amd import _C
    Bc, S, Hq, Hkv, D, dt = 5, 512, 32, 8, 64, "bfloat16"
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    q, k, v, do = _case(dev, Bc, S, S, Hq, Hkv, D, dt, seed=5)
    base = alibi_ref.default_slopes(Hq, dev)
    m = torch.stack([base.roll(3 * b) * (1.0 + 0.25 * b) for b in range(Bc)]).contiguous()       # every (b, h) its own slope
    scale = D ** -0.5
    for causal in (True, False):
        # items of the launches (include/usp_hip.h): forward 128- or 256-row tiles, dQ 256-row blocks, dK/dV 128-key blocks per
        # query-head group; all above the resident workgroups
        fwd_items = Bc * Hq * ((S + 127) // 128 if causal else (S + 255) // 256)
        assert fwd_items > cus * (2 if causal else 1) and Bc * Hq * ((S + 255) // 256) > cus and Bc * Hkv * ((S + 127) // 128) * 2 > cus
        ref = alibi_ref.ref_bwd(do, q, k, v, scale, m, causal, out_dtype=q.dtype)
        what = f"B{Bc} H{Hq}/{Hkv} S{S} causal {causal}"
        out, lse, kinds = _run_fwd(q, k, v, scale, causal, m)
        assert kinds == (("fwd_wave4",) if causal else ("fwd_wave8",)), kinds
        _check_fwd(out, lse, ref, dt, what)
        for heads in (0, 2, 4):
            grads, kinds = _run_bwd(do, q, k, v, ref, scale, causal, m, dkdv_heads=heads)
            assert {"dkdv_wave8", "dq_wave8"} <= set(kinds), kinds
            for g, r, name in zip(grads, ref[2:], ("dq", "dk", "dv")):
                assert_close(g, r, *grad_tol(dt, Hq // Hkv), f"{what} heads {heads} {name}")
        del ref
    assert _C.load().usp_attn_features() & _C.USP_ATTN_ALIBI


# ---- 5. NULL slopes are usp_flash_fwd / usp_flash_bwd; zero slopes are no bias ------------------------------------------------------
class _NullSlopes:
    """The loaded library with usp_flash_fwd / usp_flash_bwd routed through the *_alibi entry points with NULL slopes."""

    def __init__(self, L):
        self._L = L

    def usp_flash_fwd(self, a, stream):
        return self._L.usp_flash_fwd_alibi(a, None, 7, stream)

    def usp_flash_bwd(self, a, stream):
        return self._L.usp_flash_bwd_alibi(a, None, 7, stream)

    def __getattr__(self, name):
        return getattr(self._L, name)


@pytest.mark.parametrize("D,family", [(128, None), (128, "wave32"), (64, None)])
def test_null_slopes_are_the_plain_entry_points(dev, monkeypatch, D, family):
    from yunchang_amd import _C
    dt, Sq, Sk = "bfloat16", 300, 459
    q, k, v, do = _inputs(dev, Sq, Sk, D, dt)
    scale = D ** -0.5
    ref = _reference(("plain", D), do, q, k, v, scale, None, True)
    runs = []
    real = _C.load()
    for lib in (real, _NullSlopes(real)):
        monkeypatch.setattr(_C, "load", lambda lib=lib: lib)
        out, lse, fk = _run_fwd(q, k, v, scale, True, None, family=family)
        grads, bk = _run_bwd(do, q, k, v, ref, scale, True, None, family=family)
        runs.append(((out, lse) + grads, fk, bk))
    monkeypatch.setattr(_C, "load", lambda: real)
    assert runs[0][1:] == runs[1][1:], (runs[0][1:], runs[1][1:])
    if D == 128 and family is None:
        assert "dkdv_row64" in runs[1][2] and "dq_row64" in runs[1][2], runs[1][2]      # NULL slopes keep the 64-row family
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    # all-zero slopes: the ALiBi kernels, the unbiased function
    zero = torch.zeros(B, HQ, dtype=torch.float32, device=dev)
    out, lse, kinds = _run_fwd(q, k, v, scale, True, zero)
    assert set(kinds) <= _WAVE_FWD
    _check_fwd(out, lse, ref, dt, f"D{D} zero slopes")
    grads, kinds = _run_bwd(do, q, k, v, ref, scale, True, zero)
    assert {"dkdv_wave8", "dq_wave8"} <= set(kinds)
    _check_bwd(grads, ref, dt, f"D{D} zero slopes")


# ---- 6. the Python entry points ----------------------------------------------------------------------------------------------------
def test_hip_attn_func_autograd_at_a_padded_head_dim(dev):
    from yunchang_amd.kernels.attention import hip_attn_backward, hip_attn_forward, hip_attn_func
    D, dt = 96, "bfloat16"
    q, k, v, do = _case(dev, B, 300, 459, HQ, HKV, D, dt, seed=9)
    m = _slopes(dev)
    ref = alibi_ref.ref_bwd(do, q, k, v, D ** -0.5, m, True, out_dtype=q.dtype)
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    out, lse, none = hip_attn_func(*leaves, causal=True, alibi_slopes=m, return_attn_probs=True)
    assert none is None
    out.backward(do)
    assert_close(out, ref[0], *TOL[dt]["out"], "hip_attn_func out")
    assert_close(lse, ref[1], *TOL[dt]["out"], "hip_attn_func lse")
    for t, r, name in zip(leaves, ref[2:], ("dq", "dk", "dv")):
        assert_close(t.grad, r, *grad_tol(dt, 2), f"hip_attn_func {name}")
    o2, l2 = hip_attn_forward(q, k, v, causal=True, alibi_slopes=m)
    assert torch.equal(o2, out.detach()) and torch.equal(l2, lse)
    g = [torch.full_like(t, float("nan")) for t in (q, k, v)]
    hip_attn_backward(do, q, k, v, o2, l2, *g, bwd_causal=True, alibi_slopes=m)
    for a, t, name in zip(g, leaves, ("dq", "dk", "dv")):
        assert torch.equal(a, t.grad), name


def test_declines_on_the_device(dev):
    from yunchang_amd import _C
    D, dt = 128, "bfloat16"
    q, k, v, do = _inputs(dev, 300, 459, D, dt)
    m = _slopes(dev)
    scale = D ** -0.5
    for kw in (dict(softcap=30.0), dict(family="row64")):
        with pytest.raises(RuntimeError, match="code -2"):
            _run_fwd(q, k, v, scale, True, m, **kw)
        assert _C.last_launch_kinds() == ()
        lse = torch.zeros(B, HQ, 300, dtype=torch.float32, device=dev)
        grads = [torch.full(t.shape, float("nan"), dtype=torch.float32, device=dev) for t in (q, k, v)]
        with pytest.raises(RuntimeError, match="code -2"):
            _C.flash_bwd(do, q, k, v, lse, lse, *grads, scale, True, alibi=m, **kw)
        assert _C.last_launch_kinds() == () and all(bool(torch.isnan(g).all()) for g in grads)
    with pytest.raises(ValueError):
        _run_fwd(q, k, v, scale, True, m.double())
    with pytest.raises(ValueError):
        _run_fwd(q, k, v, scale, True, m.cpu())
    # unforced D = 128 runs on the two-waves-per-SIMD family (plain launches of this shape take the 64-row backward)
    _, _, kinds = _run_fwd(q, k, v, scale, True, m)
    assert kinds in (("fwd_wave8",), ("fwd_wave4",)), kinds
    ref = _reference(("blk", D, dt, True, 300, 459, "2d"), do, q, k, v, scale, m, True)
    _, kinds = _run_bwd(do, q, k, v, ref, scale, True, m)
    assert "dkdv_wave8" in kinds and "dq_wave8" in kinds and not any("row64" in x for x in kinds), kinds
    _, kinds = _run_bwd(do, q, k, v, ref, scale, True, None)
    assert "dkdv_row64" in kinds and "dq_row64" in kinds, kinds


# ---- 7. virtual ranks on one GPU ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nccl_single():
    import torch.distributed as dist
    import yunchang_amd  # noqa: F401
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29737")
    own = not dist.is_initialized()
    if own:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    yield dist
    if own:
        dist.destroy_process_group()


def _virtual_run(monkeypatch, nccl_single, dev, ud, rd, c, causal, window, slopes, repeat_backward=False):
    """Every rank of a ud x rd grid as a thread: Ulysses exchange by hand (autograd cannot run the ranks' backwards side by
    side), the slopes cut to the rank's heads, the ring forward and backward of the package with the real HipBlockBackend.
    Returns per rank (out, dq, dk, dv [, dk, dv of a second backward]) and the unsharded inputs."""
    import yunchang_amd.comm.all_to_all as A
    import yunchang_amd.ring.ring_flash_attn as R
    from yunchang_amd.kernels import get_block_backend
    from virtual_grid import VirtualGridPairwise, patch_dist, run_grid
    assert get_block_backend().name == "hip"
    monkeypatch.setenv("USP_RING_ALIBI", "global")
    monkeypatch.setenv("USP_RING_WINDOW", "global")
    grid = VirtualGridPairwise(ud, rd, nccl_single)
    patch_dist(monkeypatch, grid)
    ws, D = ud * rd, 128
    S = c * rd
    q, k, v, do = _case(dev, 1, S, S, HQ, HKV, D, "bfloat16", seed=4)
    rows = S // ws
    loc = [[t[:, r * rows:(r + 1) * rows].contiguous() for t in (q, k, v, do)] for r in range(ws)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(ws)]
    scale = D ** -0.5
    torch.cuda.synchronize()

    def rank_fn(r):
        torch.cuda.set_device(dev)
        upg, rpg = grid.groups_of(r)
        lq, lk, lv, ldo = loc[r]
        m = A.local_alibi_slopes(slopes, HQ, ud, r % ud)
        kw = dict(causal=causal, window_size=window, alibi_slopes=m)
        with torch.cuda.stream(streams[r]):
            hq, hdo = (A.heads_to_seq(t, upg, contiguous=True) for t in (lq, ldo))
            hk, hv = (A.kv_heads_to_seq(t, upg, contiguous=True) for t in (lk, lv))
            out, lse = R.ring_flash_attn_forward(rpg, hq, hk, hv, scale, **kw)
            res = []
            for _ in range(2 if repeat_backward else 1):
                dq, dk, dv = R.ring_flash_attn_backward(rpg, hdo, hq, hk, hv, out, lse, scale, **kw)
                res += [A.kv_seq_to_heads(dk, upg, HKV), A.kv_seq_to_heads(dv, upg, HKV)]
            return [A.seq_to_heads(out, upg), A.seq_to_heads(dq, upg)] + res
    res = run_grid(grid, ws, rank_fn)
    torch.cuda.synchronize()
    return res, (q, k, v, do), rows, scale


VIRTUAL = [(1, 4, True, (-1, -1)), (1, 4, False, (-1, -1)), (2, 2, True, (-1, -1)), (2, 2, False, (-1, -1)), (1, 4, True, (400, 0)),
           (1, 4, False, (100, 60))]                      # the last: blocks behind the queries (negative shifts) under a right bound


@pytest.mark.timeout(600)
@pytest.mark.parametrize("ud,rd,causal,window", VIRTUAL, ids=lambda v: str(v).replace(" ", ""))
def test_global_alibi_on_virtual_ranks(dev, nccl_single, monkeypatch, ud, rd, causal, window):
    c = 320
    twice = (ud, rd, causal, window) == (1, 4, True, (-1, -1))
    m = alibi_ref.default_slopes(HQ, dev)[None].contiguous()             # (B = 1, Hq)
    res, (q, k, v, do), rows, scale = _virtual_run(monkeypatch, nccl_single, dev, ud, rd, c, causal, window, m, twice)
    win = None if window == (-1, -1) else window
    ref = alibi_ref.ref_bwd(do, q, k, v, scale, m, causal, win, out_dtype=q.dtype)
    for r in range(ud * rd):
        sl = slice(r * rows, (r + 1) * rows)
        what = f"{ud}x{rd} causal {causal} window {window} rank {r}"
        assert_close(res[r][0], ref[0][:, sl], *TOL["bfloat16"]["out"], f"{what} out")
        for got, want, name in zip(res[r][1:4], (ref[2], ref[3], ref[4]), ("dq", "dk", "dv")):
            assert_close(got, want[:, sl], *grad_tol("bfloat16", 2), f"{what} {name}")
        if twice:
            assert torch.equal(res[r][2], res[r][4]) and torch.equal(res[r][3], res[r][5]), f"{what}: dk / dv of two identical calls"
