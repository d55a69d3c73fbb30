"""The 64-row dQ kernel's dP^T chains start from -delta: dq, densely, where that can go wrong.

`flash_bwd_dq64_kernel` no longer subtracts delta element by element (dS = P (dP - delta)): the MFMA chain that forms dP^T
starts from an accumulator tuple holding -delta of the lane's row, and the element stream multiplies by P.  Every case runs
the forced 64-row family (`family="row64"`, `"dq_row64"` asserted) on the smallest shapes that hold every path of the
change, and checks dq against oracle.usp_oracle.block_bwd with golden_util.assert_close at golden_util.TOL:

- B1 Hq4 / Hkv2 D128, Sq = Sk = 320: one full 256-row item and a ragged 64-row one -- plain tiles, masked tiles and tiles
  only the other waves of the workgroup work on, in one launch.  Causal and full, bf16 and fp16, dq_splits 0 and 2 (a key
  cut starts its chains from -delta too; the partials then sum -- delta must be counted once per key, not once per cut).
- causal Sq 320 / Sk 192: rows 0 .. 127 see no key (lse = -inf): their start constant must be 0, not NaN, and dq = 0.
- a DELTA-DOMINATED case: dO = a * out + 0.05 N(0,1), with V = N(0,1) + 4.  For N(0,1) V no `a` makes delta dominate:
  dP_j - delta = a (out . v_j - out . out) + noise terms, and out . out is the P-weighted mean of out . v_j, so
  |delta| / |dP - delta| ~ |out| whatever `a` is -- about 1 for rows that average many keys.  A component common to all
  value rows m gives out ~ m, delta ~ a |m|^2 against deviations ~ a |m|: the ratio is |m| = 4 sqrt(128) = 45 (asserted
  below: median over the rows >= 30, measured 44).  a = 0.4 puts delta at ~820 and dq at rms 0.15 - 0.3, max 2.6 - 5.4; the
  honest 16-bit model (rounding_models.bwd_16bit_model) then stays within HALF of the comparator's bound (worst error /
  bound 0.23 bf16 causal, 0.04 bf16 full, 0.09 / 0.03 fp16: test_delta_dominated_case_is_fair, CPU) and
- a MUTATION: the oracle fed delta * 1.02 (out * 1.02: delta is linear in out) misses the same comparator on that case
  by 18 - 220 x the bound, for the model on the CPU and for the kernel's result on the GPU: the case sees a lost, doubled
  or slightly wrong delta.
Measured on MI355X, worst error / bound of the kernel (the same with dq_splits 0 and 2): N(0,1) case 0.062 causal / 0.037 full
bf16, 0.045 / 0.026 fp16; delta-dominated 0.109 / 0.051 bf16, 0.147 / 0.033 fp16; against delta * 1.02 42.7 / 18.5 and 221.9 / 90.9.
"""
import functools

import numpy as np
import pytest
import torch

from golden_util import TOL, assert_close, close_mask, round_to
from oracle import usp_oracle as O
from rounding_models import bwd_16bit_model

B, HQ, HKV, D = 1, 4, 2, 128
SCALE = D ** -0.5
A_DOM, V_OFF, NOISE = 0.4, 4.0, 0.05

DTS = ["bfloat16", "float16"]


@pytest.fixture(scope="module")
def dev():
    from yunchang_amd import _C
    _C.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(kind, dt, causal, Sq=320, Sk=320):
    """(q, k, v, do, o16, lse, reference dq): computed once per case, shared, read-only."""
    rs = np.random.RandomState(5)
    q = round_to(rs.standard_normal((B, Sq, HQ, D)).astype(np.float32), dt)
    k = round_to(rs.standard_normal((B, Sk, HKV, D)).astype(np.float32), dt)
    v = rs.standard_normal((B, Sk, HKV, D))
    if kind == "delta":
        v = v + V_OFF
    v = round_to(v.astype(np.float32), dt)
    ro, rl = O.attention_ref(q, k, v, causal, SCALE)
    o16 = round_to(ro.astype(np.float32), dt)
    if kind == "delta":
        do = round_to((o16 * A_DOM + NOISE * rs.standard_normal(q.shape)).astype(np.float32), dt)
    else:
        do = round_to(rs.standard_normal(q.shape).astype(np.float32), dt)
    rdq = O.block_bwd(do, q, k, v, o16, rl, SCALE, causal)[0]
    out = (q, k, v, do, o16, rl, rdq)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mutant_dq(dt, causal):
    q, k, v, do, o16, rl, _ = case("delta", dt, causal)
    return O.block_bwd(do, q, k, v, o16 * 1.02, rl, SCALE, causal)[0]


@functools.lru_cache(maxsize=None)
def kernel_dq(kind, dt, causal, Sq, Sk, dq_splits):
    """dq of the forced 64-row dQ launch (numpy, float32)."""
    from yunchang_amd import _C
    dev = torch.device("cuda:0")
    q, k, v, do, o16, rl, _ = case(kind, dt, causal, Sq, Sk)
    t = lambda x: torch.from_numpy(np.array(x, dtype=np.float32, order="C")).to(getattr(torch, dt)).to(dev)
    tq, tk, tv, tdo, to16 = (t(x) for x in (q, k, v, do, o16))
    lse = torch.from_numpy(np.array(rl, dtype=np.float32, order="C")).to(dev)
    delta = torch.empty((B, HQ, Sq), dtype=torch.float32, device=dev)
    _C.bwd_delta(tdo, to16, delta)
    dq = torch.full_like(tq, float("nan"))
    _C.flash_bwd(tdo, tq, tk, tv, lse, delta, None, None, None, SCALE, causal, dq16=dq, family="row64", only="dq",
                 splits=(dq_splits, 0))
    kinds = _C.last_launch_kinds()
    assert "dq_row64" in kinds and "dq_wave8" not in kinds, kinds
    assert ("reduce_cuts" in kinds) == (dq_splits > 1), kinds
    return dq.float().cpu().numpy()


def _what(kind, dt, causal, Sq, Sk, dq_splits):
    return f"dq64 {kind} Sq{Sq} Sk{Sk} Hq{HQ} Hkv{HKV} causal={causal} {dt} dq_splits={dq_splits}"


def _worst(got, want, dt):
    atol, rtol = TOL[dt]["grad"]
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the delta-dominated case is what it claims to be, and fair
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dt", DTS)
def test_delta_dominated_case_is_fair(dt, causal):
    q, k, v, do, o16, rl, rdq = case("delta", dt, causal)
    g = HQ // HKV
    f8 = lambda x: x.astype(np.float64)
    dp = np.einsum("bthd,bshd->bhts", f8(do), np.repeat(f8(v), g, axis=2))
    delta = np.einsum("bthd,bthd->bht", f8(do), f8(o16))
    s = np.einsum("bthd,bshd->bhts", f8(q), np.repeat(f8(k), g, axis=2)) * SCALE
    vis = (np.arange(320)[None, :] <= np.arange(320)[:, None]) if causal else np.ones((320, 320), bool)
    p = np.where(vis, np.exp(s - rl[..., None]), 0.0)
    typical = np.sqrt((p * (dp - delta[..., None]) ** 2).sum(-1))               # P-weighted rms of dP - delta, per row
    rows = typical > 0                                                          # (a causal row 0 sees one key: dP = delta)
    ratio = float(np.median(np.abs(delta)[rows] / typical[rows]))
    assert ratio >= 30, f"|delta| is {ratio:.1f} x the typical |dP - delta|"
    atol, rtol = TOL[dt]["grad"]
    model = bwd_16bit_model(do, q, k, v, o16, rl, SCALE, causal, dt, False)[0]
    print(f"[dq64-delta] {dt} causal={causal}: |delta| / |dP - delta| median {ratio:.1f}, honest model worst error / bound "
          f"{_worst(model, rdq, dt):.3f}, against the mutated oracle {_worst(model, mutant_dq(dt, causal), dt):.1f}")
    assert_close(model, rdq, atol / 2, rtol / 2, "honest 16-bit model, half of the bound")
    assert not close_mask(model, mutant_dq(dt, causal), atol, rtol)[0].all(), "the case does not see delta * 1.02"


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dq_splits", [0, 2])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dt", DTS)
def test_dq64_plain_masked_and_ragged_tiles(dev, dt, causal, dq_splits):
    key = ("normal", dt, causal, 320, 320, dq_splits)
    got, want = kernel_dq(*key), case("normal", dt, causal)[6]
    print(f"[dq64-delta] {_what(*key)}: worst error / bound {_worst(got, want, dt):.3f}")
    assert_close(got, want, *TOL[dt]["grad"], _what(*key))


@pytest.mark.gpu
@pytest.mark.parametrize("dq_splits", [0, 2])
@pytest.mark.parametrize("dt", DTS)
def test_dq64_rows_that_see_no_key(dev, dt, dq_splits):
    key = ("normal", dt, True, 320, 192, dq_splits)
    rl, want = case("normal", dt, True, 320, 192)[5:7]
    dead = ~np.isfinite(rl[0, 0])
    assert dead[:128].all() and not dead[128:].any()
    got = kernel_dq(*key)
    assert (got[:, :128] == 0).all(), _what(*key) + ": rows without a visible key must give dq = 0"
    assert_close(got, want, *TOL[dt]["grad"], _what(*key))


@pytest.mark.gpu
@pytest.mark.parametrize("dq_splits", [0, 2])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dt", DTS)
def test_dq64_delta_dominated(dev, dt, causal, dq_splits):
    key = ("delta", dt, causal, 320, 320, dq_splits)
    got, want = kernel_dq(*key), case("delta", dt, causal)[6]
    print(f"[dq64-delta] {_what(*key)}: worst error / bound {_worst(got, want, dt):.3f}")
    assert_close(got, want, *TOL[dt]["grad"], _what(*key))


@pytest.mark.gpu
@pytest.mark.parametrize("dq_splits", [0, 2])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dt", DTS)
def test_dq64_delta_dominated_sees_a_wrong_delta(dev, dt, causal, dq_splits):
    """The kernel's dq against the oracle fed delta * 1.02: the same comparator must refuse it."""
    key = ("delta", dt, causal, 320, 320, dq_splits)
    got = kernel_dq(*key)
    print(f"[dq64-delta] {_what(*key)}: worst error / bound against delta * 1.02: {_worst(got, mutant_dq(dt, causal), dt):.1f}")
    with pytest.raises(AssertionError):
        assert_close(got, mutant_dq(dt, causal), *TOL[dt]["grad"], _what(*key) + " against delta * 1.02")
