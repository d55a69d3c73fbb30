"""Randomised GPU parity sweep: many small ragged shapes (dense and packed, MHA and GQA, causal and full,
Sq != Sk, every head dim, both dtypes) through the C ABI against the CPU oracle, every call launched twice and
required to be bit-identical (the kernels are deterministic; a difference means a race).  Sizes keep the fp64
oracle at a few milliseconds per case.  Seeds are fixed: failures reproduce.  `test_fuzz_features` puts softcap, ALiBi and dropout
(one a case) through the shapes of the shifted sweep, the second launch with an independent strided layout per tensor.
Attention sinks and the document mask have sweeps of their own on these shapes: tests/test_gpu_fuzz_sink_doc.py."""
import numpy as np
import pytest
import torch

from golden_util import TOL, assert_close, long_sum_atol, round_to
from oracle import usp_oracle as O

pytestmark = pytest.mark.gpu

import os
_N_DENSE = int(os.environ.get("USP_FUZZ_DENSE", "28"))      # larger sweeps: USP_FUZZ_DENSE=400 USP_FUZZ_PACKED=200
_N_PACKED = int(os.environ.get("USP_FUZZ_PACKED", "14"))


@pytest.fixture(scope="module")
def dev():
    from yunchang_amd import _C
    _C.load()
    return torch.device("cuda:0")


def _t(x, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(getattr(torch, dt)).to(dev)


def _f(t):
    return t.detach().float().cpu().numpy()


def _dense_case(rs):
    D = int(rs.choice([32, 64, 128]))
    dt = str(rs.choice(["bfloat16", "float16"]))
    Hkv = int(rs.choice([1, 2, 3]))
    Hq = Hkv * int(rs.choice([1, 2, 4]))
    B = int(rs.choice([1, 2, 3]))
    Sq = int(rs.randint(1, 700))
    Sk = Sq if rs.rand() < 0.5 else int(rs.randint(1, 700))
    causal = bool(rs.rand() < 0.6)
    # (drawn last, so that the shapes of the earlier rounds' seeds stay what they were)  a third of the cases carry a
    # sliding window, a third the K split of the forward and cuts of the two backward launches (ABI v5)
    win = None
    if rs.rand() < 0.33:
        win = (int(rs.choice([-1, 0, 1, 17, 64, 200, 1000])), int(rs.choice([-1, 0, 3, 40])))
        if win == (-1, -1):
            win = (33, 0)
    ks, cuts = 0, (0, 0)
    if rs.rand() < 0.33:
        ks, cuts = int(rs.choice([2, 3, 5, 8])), (int(rs.choice([0, 2, 3, 8])), int(rs.choice([0, 2, 4])))
    return B, Sq, Sk, Hq, Hkv, D, causal, dt, win, ks, cuts


@pytest.mark.parametrize("seed", range(_N_DENSE))
def test_fuzz_dense(dev, seed):
    rs = np.random.RandomState(1000 + seed)
    _run_dense(dev, rs, _dense_case(rs))


_N_ROW64 = int(os.environ.get("USP_FUZZ_ROW64", "16"))      # larger sweeps: USP_FUZZ_ROW64=300


def _row64_case(rs):
    """Shapes the one-wave-per-SIMD BACKWARD kernels serve by the library's own dispatch (D = 128, dense, no window, no
    cuts; both dtypes): they take every such launch, however small.  The 4 x 64 FORWARD is dispatched from 256 work items
    up, which no shape here has -- this sweep's forward runs on the 4-wave kernel; the forced sweep of
    tests/test_gpu_row64.py is the one that puts ragged shapes through `flash_fwd64_kernel`.  Longer sequences than the
    general sweep: several 256-row query blocks and 128-key blocks per head, ragged ends, Sq != Sk in both directions,
    GQA groups up to 8."""
    dt = str(rs.choice(["bfloat16", "bfloat16", "float16"]))
    Hkv = int(rs.choice([1, 2]))
    Hq = Hkv * int(rs.choice([1, 2, 4, 8]))
    B = int(rs.choice([1, 2]))
    Sq = int(rs.choice([rs.randint(1, 130), rs.randint(130, 1400)]))
    Sk = Sq if rs.rand() < 0.5 else int(rs.choice([rs.randint(1, 130), rs.randint(130, 1400)]))
    causal = bool(rs.rand() < 0.6)
    return B, Sq, Sk, Hq, Hkv, 128, causal, dt, None, 0, (0, 0)


@pytest.mark.parametrize("seed", range(_N_ROW64))
def test_fuzz_64row_kernels(dev, seed):
    rs = np.random.RandomState(5000 + seed)
    _run_dense(dev, rs, _row64_case(rs))


_N_SHIFTED = int(os.environ.get("USP_FUZZ_SHIFTED", "16"))  # larger sweeps: USP_FUZZ_SHIFTED=300


def _shifted_case(rs):
    """The shapes of `_dense_case` with a bound always (causal or a window), a shift on tile edges, beside them, half a
    sequence away and past the last key, K split / cuts in a third of the cases, `dkdv_heads` from the divisors of the group."""
    B, Sq, Sk, Hq, Hkv, D, causal, dt, win, ks, cuts = _dense_case(rs)
    if not causal and win is None:
        if rs.rand() < 0.5:
            causal = True
        else:
            win = (int(rs.choice([0, 1, 17, 64, 200])), int(rs.choice([-1, 0, 3, 40])))
    shift = int(rs.choice([0, 1, -1, 63, -63, 64, -64, 65, -65, Sq // 2, -(Sq // 2), Sk + 5, -(Sk + 5)]))
    G = Hq // Hkv
    heads = int(rs.choice([g for g in range(1, G + 1) if G % g == 0]))
    family = str(rs.choice(["auto", "wave32", "row64"]))    # (the 64-row family: D 128 without a left bound)
    if family == "row64" and (D != 128 or (win is not None and win[0] >= 0)):
        family = "wave32"
    return (B, Sq, Sk, Hq, Hkv, D, causal, dt, win, ks, cuts), shift, heads, (None if family == "auto" else family)


@pytest.mark.parametrize("seed", range(_N_SHIFTED))
def test_fuzz_shifted(dev, seed):
    """A shifted diagonal (USP_ATTN_SHIFT) on N(0,1) inputs against tests/shift_ref.py: the bookkeeping of rows, tiles and whole
    launches without a visible key across every head dim and both dispatches (which key is the last visible one is pinned on
    needle inputs, tests/test_gpu_needle.py)."""
    rs = np.random.RandomState(9000 + seed)
    case, shift, heads, family = _shifted_case(rs)
    _run_dense(dev, rs, case, shift=shift, dkdv_heads=heads, family=family)


def _shift_reference(tq, tk, tv, tdo, scale, causal, win, shift):
    """(out, lse, dq, dk, dv) in fp64 from tests/shift_ref.py on the device, as numpy; the backward from the 16-bit-rounded out."""
    import shift_ref
    ro, rl = shift_ref.ref_fwd(tq, tk, tv, scale, causal, win, shift)
    g = shift_ref.ref_bwd(tdo, tq, tk, tv, ro.to(tq.dtype), rl, scale, causal, win, shift)
    return tuple(t.cpu().numpy() for t in (ro, rl) + tuple(g))


def _run_dense(dev, rs, case, shift=None, dkdv_heads=0, family=None):
    from yunchang_amd import _C
    B, Sq, Sk, Hq, Hkv, D, causal, dt, win, ks, cuts = case
    what = f"B{B} Sq{Sq} Sk{Sk} Hq{Hq} Hkv{Hkv} D{D} causal={causal} {dt} window={win} k_splits={ks} cuts={cuts}"
    wkw = {} if win is None else {"window": win}
    if shift is not None:
        what += f" shift={shift} dkdv_heads={dkdv_heads} family={family}"
    q, k, v, do = (round_to(rs.standard_normal(s).astype(np.float32), dt)
                   for s in [(B, Sq, Hq, D), (B, Sk, Hkv, D), (B, Sk, Hkv, D), (B, Sq, Hq, D)])
    tq, tk, tv, tdo = (_t(x, dt, dev) for x in (q, k, v, do))
    scale = D ** -0.5
    if shift is None:
        ro, rl = O.attention_ref(q, k, v, causal, scale, **wkw)
    else:
        ro, rl, rdq, rdk, rdv = _shift_reference(tq, tk, tv, tdo, scale, causal, win, shift)
        wkw = dict(wkw, shift=shift, family=family)
    runs = []
    for _ in range(2):
        out = torch.full((B, Sq, Hq, D), float("nan"), dtype=tq.dtype, device=dev)
        lse = torch.full((B, Hq, Sq), float("nan"), dtype=torch.float32, device=dev)
        _C.flash_fwd(tq, tk, tv, scale, causal, lse, out=out, interleave=len(runs) == 1, k_splits=ks, **wkw)
        runs.append((_f(out), _f(lse)))
    assert np.array_equal(runs[0][0], runs[1][0], equal_nan=True) and np.array_equal(runs[0][1], runs[1][1]), what
    fin = np.isfinite(rl)
    assert (np.isfinite(runs[0][1]) == fin).all(), what + ": empty rows must give lse = -inf"
    assert_close(runs[0][0], ro, *TOL[dt]["out"], what + " out")
    assert_close(runs[0][1][fin], rl[fin], 2e-3, 1e-4, what + " lse")
    o16 = round_to(ro.astype(np.float32), dt)
    if shift is None:
        rdq, rdk, rdv = O.block_bwd(do, q, k, v, o16, rl, scale, causal, **wkw)
    lse_t = torch.from_numpy(np.ascontiguousarray(rl, dtype=np.float32)).to(dev)
    delta = torch.empty((B, Hq, Sq), dtype=torch.float32, device=dev)
    _C.bwd_delta(tdo, _t(o16, dt, dev), delta)
    grads = []
    for _ in range(2):
        dq, dk, dv = (torch.full_like(t, float("nan")) for t in (tq, tk, tv))
        _C.flash_bwd(tdo, tq, tk, tv, lse_t, delta, None, None, None, scale, causal, dq16=dq, dk16=dk, dv16=dv,
                     interleave=len(grads) == 1, splits=cuts, dkdv_heads=dkdv_heads, **wkw)
        grads.append([_f(x) for x in (dq, dk, dv)])
    for a_, b_, n_ in zip(grads[0], grads[1], ("dq", "dk", "dv")):
        assert np.array_equal(a_, b_), f"{what}: {n_} differs between two launches"
    for g_, r_, n_ in zip(grads[0], (rdq, rdk, rdv), ("dq", "dk", "dv")):
        # long sums of 16-bit-rounded products (dK / dV sum Sq * G rows, dQ sums Sk keys): golden_util.long_sum_atol
        atol, rtol = TOL[dt]["grad"]
        atol = long_sum_atol(atol, Sk if n_ == "dq" else Sq * (Hq // Hkv), r_)
        assert_close(g_, r_, atol, rtol, f"{what} {n_}")


@pytest.mark.parametrize("seed", range(_N_PACKED))
def test_fuzz_packed(dev, seed):
    from yunchang_amd import _C
    rs = np.random.RandomState(2000 + seed)
    D = int(rs.choice([32, 64, 128]))
    dt = str(rs.choice(["bfloat16", "float16"]))
    Hkv = int(rs.choice([1, 2]))
    Hq = Hkv * int(rs.choice([1, 2, 4]))
    n = int(rs.randint(1, 7))
    lq = [int(x) for x in rs.randint(1, 400, size=n)]
    same = rs.rand() < 0.6
    lk = lq if same else [int(x) for x in rs.randint(1, 400, size=n)]
    causal = bool(rs.rand() < 0.7)
    what = f"lens_q={lq} lens_k={lk} Hq{Hq} Hkv{Hkv} D{D} causal={causal} {dt}"
    Tq, Tk = sum(lq), sum(lk)
    q, k, v, do = (round_to(rs.standard_normal(s).astype(np.float32), dt)
                   for s in [(Tq, Hq, D), (Tk, Hkv, D), (Tk, Hkv, D), (Tq, Hq, D)])
    tq, tk, tv, tdo = (_t(x, dt, dev) for x in (q, k, v, do))
    cq, ck = np.concatenate([[0], np.cumsum(lq)]), np.concatenate([[0], np.cumsum(lk)])
    sq = torch.tensor(np.stack([cq[:-1], lq], 1), dtype=torch.int32, device=dev)
    sk = torch.tensor(np.stack([ck[:-1], lk], 1), dtype=torch.int32, device=dev)
    scale = D ** -0.5
    ro = np.zeros((Tq, Hq, D)); rl = np.zeros((Hq, Tq))
    rdq = np.zeros((Tq, Hq, D)); rdk = np.zeros((Tk, Hkv, D)); rdv = np.zeros((Tk, Hkv, D))
    for i in range(n):
        a, b, c, d = cq[i], cq[i + 1], ck[i], ck[i + 1]
        o_i, l_i = O.block_fwd(q[None, a:b], k[None, c:d], v[None, c:d], scale, causal)
        ro[a:b], rl[:, a:b] = o_i[0], l_i[0]
    o16 = round_to(ro.astype(np.float32), dt)
    for i in range(n):
        a, b, c, d = cq[i], cq[i + 1], ck[i], ck[i + 1]
        g = O.block_bwd(do[None, a:b], q[None, a:b], k[None, c:d], v[None, c:d], o16[None, a:b], rl[None, :, a:b],
                        scale, causal)
        rdq[a:b], rdk[c:d], rdv[c:d] = g[0][0], g[1][0], g[2][0]
    runs = []
    for _ in range(2):
        out = torch.full((Tq, Hq, D), float("nan"), dtype=tq.dtype, device=dev)
        lse = torch.full((Hq, Tq), float("nan"), dtype=torch.float32, device=dev)
        # second launch: the one-item-per-workgroup shape used beside transfers (USP_LAUNCH_INTERLEAVE)
        _C.flash_fwd_packed(tq, tk, tv, sq, sk, max(lq), max(lk), scale, causal, lse, out=out, interleave=len(runs) == 1)
        runs.append((_f(out), _f(lse)))
    assert np.array_equal(runs[0][0], runs[1][0], equal_nan=True) and np.array_equal(runs[0][1], runs[1][1]), what
    fin = np.isfinite(rl)
    assert (np.isfinite(runs[0][1]) == fin).all(), what
    assert_close(runs[0][0], ro, *TOL[dt]["out"], what + " out")
    assert_close(runs[0][1][fin], rl[fin], 2e-3, 1e-4, what + " lse")
    lse_t = torch.from_numpy(np.ascontiguousarray(rl, dtype=np.float32)).to(dev)
    delta = torch.empty((Hq, Tq), dtype=torch.float32, device=dev)
    _C.bwd_delta(tdo[None], _t(o16, dt, dev)[None], delta[None])
    grads = []
    for _ in range(2):
        dq, dk, dv = (torch.full_like(t, float("nan")) for t in (tq, tk, tv))
        _C.flash_bwd_packed(tdo, tq, tk, tv, lse_t, delta, sq, sk, max(lq), max(lk), None, None, None, scale, causal,
                            dq16=dq, dk16=dk, dv16=dv, interleave=len(grads) == 1)
        grads.append([_f(x) for x in (dq, dk, dv)])
    for a_, b_, n_ in zip(grads[0], grads[1], ("dq", "dk", "dv")):
        assert np.array_equal(a_, b_), f"{what}: {n_} differs between two launches"
    for g_, r_, n_ in zip(grads[0], (rdq, rdk, rdv), ("dq", "dk", "dv")):
        assert_close(g_, r_, *TOL[dt]["grad"], f"{what} {n_}")
    assert int(_C.sched_block(dev).abs().sum()) == 0, "the work-queue control block must be left zeroed"


_N_FEATURES = int(os.environ.get("USP_FUZZ_FEATURES", "36"))  # 12 per feature; larger sweeps: USP_FUZZ_FEATURES=600
_FEATURES = ("softcap", "alibi", "dropout")


def _feature_case(rs, seed):
    """The shapes of `_shifted_case` (the forced 64-row family declines all three features: the library's own dispatch or
    "wave32") plus ONE feature, in rotation by seed; every extra draw comes after the shape's."""
    case, shift, heads, family = _shifted_case(rs)
    B, Hq = case[0], case[3]
    family = "wave32" if family == "row64" else family
    feature = _FEATURES[seed % 3]
    if feature == "softcap":
        par = float(rs.choice([2.5, 6.0, 30.0]))
    elif feature == "alibi":
        par = (2.0 ** (-8.0 * rs.rand(*((B, Hq) if rs.rand() < 0.5 else (Hq,))))).astype(np.float32)     # log-uniform in [2^-8, 1]
        if rs.rand() < 1.0 / 3:
            par[..., int(rs.randint(Hq))] = 0.0                 # one head without a bias
    else:
        par = (float(rs.choice([0.1, 0.25, 0.5])), (int(rs.randint(0, 1 << 32, dtype=np.uint64)) << 32) | int(rs.randint(0, 1 << 32, dtype=np.uint64)),
               4 * int(rs.randint(0, 1 << 28)), 4 * int(rs.randint(0, 1 << 28)), int(rs.randint(0, 64)))
    return case, shift, heads, family, feature, par


def _feature_reference(feature, par, tq, tk, tv, tdo, scale, causal, win, shift):
    """(out, lse, dq, dk, dv) in fp64 on the device: tests/shift_ref.py with softcap, tests/alibi_ref.py, tests/dropout_ref.py; the
    backward from the 16-bit-rounded out."""
    import alibi_ref
    import dropout_ref
    import shift_ref
    if feature == "softcap":
        ro, rl = shift_ref.ref_fwd(tq, tk, tv, scale, causal, win, shift, softcap=par)
        return (ro, rl) + tuple(shift_ref.ref_bwd(tdo, tq, tk, tv, ro.to(tq.dtype), rl, scale, causal, win, shift, softcap=par))
    if feature == "alibi":
        return alibi_ref.ref_bwd(tdo, tq, tk, tv, scale, torch.from_numpy(par).to(tq.device), causal, win, shift, out_dtype=tq.dtype)
    return dropout_ref.ref_bwd(tdo, tq, tk, tv, scale, par[0], par[1], par[2:], causal, win, shift, out_dtype=tq.dtype)


def _feature_tol(feature, par, dt, G, name):
    """(atol, rtol) as the feature's own GPU test has them: tests/test_gpu_softcap.py (TOL / grad_tol, the LSE as _run_dense),
    tests/test_gpu_alibi.py (out and LSE at TOL[dt]["out"], gradients at grad_tol(dt, G)), tests/test_gpu_dropout.py:_tol (atol x
    256/t for out and the gradients, the plain tolerance for the LSE)."""
    import dropout_ref
    from golden_util import grad_tol
    if name == "lse":
        return (2e-3, 1e-4) if feature == "softcap" else TOL[dt]["out"]
    atol, rtol = TOL[dt]["out"] if name == "out" else grad_tol(dt, G)
    return (atol * dropout_ref.rescale(par[0]), rtol) if feature == "dropout" else (atol, rtol)


def _err_line(tag, what, name, got, want, atol, rtol):
    from golden_util import close_mask
    _, err = close_mask(got, want, atol, rtol)
    frac = float((err / (atol + rtol * want.abs().to(err.dtype))).nan_to_num(0.0).max())
    print(f"[{tag}-err] {what} {name}: {frac:.3f} of tolerance")


@pytest.mark.parametrize("seed", range(_N_FEATURES))
def test_fuzz_features(dev, seed):
    """softcap, ALiBi and dropout on the ragged shapes, odd GQA groups, cuts and shifts of the dense sweeps, one feature a case,
    against their fp64 references; every call launched twice and required bit-identical, the second launch with
    interleave=True and every tensor of the call an independently drawn strided view inside one sentinel arena
    (tests/layout_util.py), which must be intact afterwards."""
    from yunchang_amd import _C
    import layout_util as LU
    rs = np.random.RandomState(13000 + seed)
    case, shift, heads, family, feature, par = _feature_case(rs, seed)
    B, Sq, Sk, Hq, Hkv, D, causal, dt, win, ks, cuts = case
    G = Hq // Hkv
    shown = par if feature != "alibi" else f"slopes {par.shape} zero head {bool((par == 0).any())}"
    what = (f"{feature} {shown} B{B} Sq{Sq} Sk{Sk} Hq{Hq} Hkv{Hkv} D{D} causal={causal} {dt} window={win} k_splits={ks} cuts={cuts} "
            f"shift={shift} dkdv_heads={heads} family={family}")
    q, k, v, do = (round_to(rs.standard_normal(s).astype(np.float32), dt)
                   for s in [(B, Sq, Hq, D), (B, Sk, Hkv, D), (B, Sk, Hkv, D), (B, Sq, Hq, D)])
    if feature == "softcap":
        q = round_to(q * 4.0, dt)                             # exact: the cap bites (layout_util.make_inputs)
    tq, tk, tv, tdo = (_t(x, dt, dev) for x in (q, k, v, do))
    scale = D ** -0.5
    ro, rl, rdq, rdk, rdv = _feature_reference(feature, par, tq, tk, tv, tdo, scale, causal, win, shift)
    fkw = {"softcap": dict(softcap=par), "alibi": dict(alibi=torch.from_numpy(par).to(dev)) if feature == "alibi" else None,
           "dropout": dict(dropout=par)}[feature]
    wkw = dict(fkw, shift=shift, family=family, **({} if win is None else {"window": win}))
    lay = lambda name: LU.draw_layout(rs, LU.ROLE[name], B)      # (drawn last: after the shape, the feature and the inputs)
    arena = LU.Arena(dev)
    dtype = tq.dtype
    # ---- forward: contiguous, then interleave + an independent layout per tensor
    out = torch.full((B, Sq, Hq, D), float("nan"), dtype=dtype, device=dev)
    lse = torch.full((B, Hq, Sq), float("nan"), dtype=torch.float32, device=dev)
    _C.flash_fwd(tq, tk, tv, scale, causal, lse, out=out, k_splits=ks, **wkw)
    kinds = _C.last_launch_kinds()
    assert kinds and not any("row64" in x for x in kinds), (what, kinds)
    sq, sk, sv, sdo = (LU.place(t, lay(n), arena, n) for t, n in ((tq, "q"), (tk, "k"), (tv, "v"), (tdo, "dout")))
    out2 = LU.blank((B, Sq, Hq, D), dtype, lay("out"), arena, "out")
    lse2 = LU.blank((B, Hq, Sq), torch.float32, lay("lse"), arena, "lse")
    _C.flash_fwd(sq, sk, sv, scale, causal, lse2, out=out2, interleave=True, k_splits=ks, **wkw)
    assert torch.equal(LU.raw_bits(out), LU.raw_bits(out2)) and torch.equal(LU.raw_bits(lse), LU.raw_bits(lse2)), \
        f"{what}: the forward differs between two launches"
    fin = torch.isfinite(rl)
    assert bool((torch.isfinite(lse) == fin).all()), what + ": empty rows must give lse = -inf"
    tag = f"fuzz-{feature}"
    _err_line(tag, what, "out", out, ro, *_feature_tol(feature, par, dt, G, "out"))
    assert_close(out, ro, *_feature_tol(feature, par, dt, G, "out"), what + " out")
    assert_close(lse[fin], rl[fin], *_feature_tol(feature, par, dt, G, "lse"), what + " lse")
    if feature == "dropout":                                   # the mask did something in every row that sees more than 8 keys
        import shift_ref
        plain = torch.full_like(out, float("nan"))
        _C.flash_fwd(tq, tk, tv, scale, causal, torch.empty_like(lse), out=plain, k_splits=ks,
                     **{k_: v_ for k_, v_ in wkw.items() if k_ != "dropout"})
        many = shift_ref.visible(Sq, Sk, causal, win, shift, dev).sum(-1) > 8
        same = (out == plain).all(-1)[:, many]                # (B, rows, Hq)
        assert not bool(same.any()), f"{what}: {int(same.sum())} rows with more than 8 keys equal the p = 0 result"
    # ---- backward: lse from the reference, delta from the 16-bit-rounded reference out
    lse_t = rl.to(torch.float32)
    delta = torch.empty((B, Hq, Sq), dtype=torch.float32, device=dev)
    _C.bwd_delta(tdo, ro.to(dtype), delta)
    g1 = [torch.full_like(t, float("nan")) for t in (tq, tk, tv)]
    _C.flash_bwd(tdo, tq, tk, tv, lse_t, delta, None, None, None, scale, causal, dq16=g1[0], dk16=g1[1], dv16=g1[2],
                 splits=cuts, dkdv_heads=heads, **wkw)
    kinds = _C.last_launch_kinds()
    assert {"dkdv_wave8", "dq_wave8"} <= set(kinds) and not any("row64" in x for x in kinds), (what, kinds)
    slse, sdelta = LU.place(lse_t, lay("lse"), arena, "lse_in"), LU.place(delta, lay("delta"), arena, "delta")
    g2 = [LU.blank(tuple(t.shape), dtype, lay(n), arena, n) for t, n in ((tq, "dq16"), (tk, "dk16"), (tv, "dv16"))]
    _C.flash_bwd(sdo, sq, sk, sv, slse, sdelta, None, None, None, scale, causal, dq16=g2[0], dk16=g2[1], dv16=g2[2],
                 interleave=True, splits=cuts, dkdv_heads=heads, **wkw)
    for a_, b_, n_ in zip(g1, g2, ("dq", "dk", "dv")):
        assert torch.equal(LU.raw_bits(a_), LU.raw_bits(b_)), f"{what}: {n_} differs between two launches"
    bad = arena.violations()
    assert not bad, f"{what}: written outside the views: {bad}"
    assert arena.unchanged(), what + ": an input view was modified"
    for g_, r_, n_ in zip(g1, (rdq, rdk, rdv), ("dq", "dk", "dv")):
        # long sums of 16-bit-rounded products (dK / dV sum Sq * G rows, dQ sums Sk keys): golden_util.long_sum_atol
        atol, rtol = _feature_tol(feature, par, dt, G, n_)
        atol = long_sum_atol(atol, Sk if n_ == "dq" else Sq * G, r_)
        _err_line(tag, what, n_, g_, r_, atol, rtol)
        assert_close(g_, r_, atol, rtol, f"{what} {n_}")
