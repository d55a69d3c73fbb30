"""Value-range inputs (tests/range_inputs.py) are fair and sharp -- without a GPU.

Fair: for every case tests/test_gpu_range.py runs, the fp64 reference passes against the HONEST 16-bit model
(tests/rounding_models.py: P rounded before P V and before dS is formed, dS rounded before dQ / dK; K NOT pre-scaled) with
at most half of every stated bound, every element compared.  A case that did not was re-tuned (amplitude of dout, its
common part, the seed), never given a wider bound.  For `steps`, P relative to the reference max stays below 2^8.

Sharp: the same comparator fails the models of kernels that are subtly wrong in the ways these inputs were made for."""
import functools

import numpy as np
import pytest

import needle_inputs as NI
import range_inputs as RI
import rounding_models as RM
from golden_util import round_to
from oracle import usp_oracle as O


@functools.lru_cache(maxsize=None)
def _case(cid):
    c = RI.BY_ID[cid]
    ns = RI.make(c)
    return c, ns, RI.reference(c, ns, bwd=c.kind != "steps")


def _fwd(cid, scale_mul=1.0, **kw):
    c, ns, want = _case(cid)
    out, lse, p_max = RM.fwd_16bit_model(ns.q, ns.k, ns.v, ns.scale * scale_mul, c.causal, c.dt, softcap=c.softcap, **kw)
    ver = RI.verdicts(c, ns, dict(out=out, lse=lse), want)
    return {n_: r for n_, (_, r) in ver.items()}, p_max


def _bwd(cid, prescale_k=False, scale_mul=1.0, epilogue_div=1.0):
    c, ns, want = _case(cid)
    dq, dk, dv = RM.bwd_16bit_model(ns.do, ns.q, ns.k, ns.v, want["o16"], want["lse"], ns.scale * scale_mul, c.causal, c.dt,
                                    prescale_k, softcap=c.softcap)
    ver = RI.verdicts(c, ns, dict(dq=dq / epilogue_div, dk=dk / epilogue_div, dv=dv), want)
    return {n_: r for n_, (_, r) in ver.items()}


# ---------------------------------------------------------------------------------------------------------------------
# conditions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in RI.ALL])
def test_honest_16bit_model_keeps_half_of_every_bound(cid):
    """Every case of the GPU file (the packed one: test_honest_16bit_model_on_the_packed_case)."""
    c, ns, want = _case(cid)
    for x in (ns.q, ns.k, ns.v, ns.do):
        assert np.array_equal(round_to(x, c.dt), x) and np.isfinite(x).all(), cid + ": inputs must be exact in the 16-bit type"
    assert all(np.isfinite(w[np.isfinite(want["lse"])] if n_ == "lse" else w).all() for n_, w in want.items()), cid
    ratios, p_max = _fwd(cid)
    if c.kind == "steps":
        assert p_max <= 2.0 ** RM.K_THR * (1 + 1e-9), (cid, p_max)
    if c.kind != "steps":
        ratios.update(_bwd(cid))
    assert all(r <= 0.5 for r in ratios.values()), (cid, ratios)


def test_honest_16bit_model_on_the_packed_case():
    """range_inputs.PACKED: every sequence a causal problem of its own, judged together as the GPU test judges them."""
    c = RI.PACKED
    ns = RI.make(c)
    want = RI.packed_reference(c, ns)
    got = {n_: np.zeros_like(want[n_]) for n_ in ("out", "lse", "dq", "dk", "dv")}
    for s0, n in RI.PACKED_SEQS:
        sl = slice(s0, s0 + n)
        out, lse, _ = RM.fwd_16bit_model(ns.q[:, sl], ns.k[:, sl], ns.v[:, sl], ns.scale, True, c.dt)
        dq, dk, dv = RM.bwd_16bit_model(ns.do[:, sl], ns.q[:, sl], ns.k[:, sl], ns.v[:, sl], want["o16"][:, sl],
                                        want["lse"][:, :, sl], ns.scale, True, c.dt, False)
        got["out"][:, sl], got["lse"][:, :, sl], got["dq"][:, sl], got["dk"][:, sl], got["dv"][:, sl] = out, lse, dq, dk, dv
    ratios = {n_: r for n_, (_, r) in RI.verdicts(c, ns, got, want).items()}
    assert all(r <= 0.5 for r in ratios.values()), ratios


def test_fp16_edge_judges_every_dq_channel_at_its_own_scale():
    """With the large K channel only that channel of dq is normalised further (2^-10); on the other 127 channels the
    honest model sits where the tame case's does, not orders of magnitude below the bound."""
    c, ns, want = _case("edge-5.5-bigk")
    assert (ns.norm["dq"] == 4.0).sum() == c.D - 1 and ns.norm["dq"][RI.EDGE_CH] == 2.0 ** -10
    dq, _, _ = RM.bwd_16bit_model(ns.do, ns.q, ns.k, ns.v, want["o16"], want["lse"], ns.scale, c.causal, c.dt, False)
    other = np.arange(c.D) != RI.EDGE_CH
    ns2 = RI.make(c)
    ns2.norm = dict(dq=4.0)
    r_other = RI.verdicts(c, ns2, dict(dq=dq[..., other]), dict(dq=want["dq"][..., other]))["dq"][1]
    assert 0.05 < r_other <= 0.5, r_other


@pytest.mark.parametrize("cid", [c.id for c in RI.SCALED if c.kind == "pair"])
def test_exact_pairs_are_the_same_problem(cid):
    """The fp64 result of the launched problem, times `mul`, is the fp64 result of the unscaled problem to 1e-12."""
    c, ns, want = _case(cid)
    ro, rl = O.attention_ref(ns.q, ns.k, ns.v, c.causal, ns.scale)
    dq, dk, dv = O.block_bwd(ns.do, ns.q, ns.k, ns.v, want["o16"], rl, ns.scale, c.causal)
    for n_, x in dict(out=ro, lse=rl, dq=dq, dk=dk, dv=dv).items():
        np.testing.assert_allclose(x * ns.mul.get(n_, 1.0), want[n_], rtol=1e-11, atol=1e-12 * np.abs(want[n_]).max(), err_msg=n_)
    assert abs(np.log2(ns.scale / c.D ** -0.5)) >= 6 or "subnormal" in cid


@pytest.mark.parametrize("cid", [c.id for c in RI.SCALED if c.kind == "scale"])
def test_independent_scales_keep_the_scores_within_15_nat(cid):
    c, ns, _ = _case(cid)
    kk = np.repeat(ns.k, c.Hq // c.Hkv, axis=2).astype(np.float64)
    s = np.einsum("bthd,bshd->bhts", ns.q.astype(np.float64), kk) * ns.scale
    assert 4.0 < np.abs(s).max() <= 15.0, (cid, np.abs(s).max())
    assert abs(ns.scale / c.D ** -0.5 - 1) > 0.5


def test_subnormal_pair_puts_scaled_k_in_the_fp16_subnormal_range():
    c, ns, _ = _case("pair-k-subnormal")
    kc = np.abs(ns.k.astype(np.float64)) * ns.scale * RM.LOG2E
    assert np.median(kc) < 2.0 ** -14 and (np.abs(ns.k) < 2.0 ** -14).mean() > 0.05, "K * scale * log2(e) must be subnormal in fp16"


def test_steps_rows_of_one_wave_jump_and_stay():
    """Inside every 32 consecutive rows of the block some rows' aligned score rises by more than kThr = 8 log2 units from
    tile to tile and others' by less (7.5 and 8.5 per tile at multiplier 1: one on each side)."""
    for cid, lo, hi in (("rise7.5-row64-b128", 7.5, 7.5 * 1.25), ("rise8.5-wave32-b128", 8.5 * 0.875, 8.5)):
        c, ns, _ = _case(cid)
        r0, r1 = RI.step_rows(c)
        assert lo < RM.K_THR < hi
        s2 = np.einsum("thd,sd->hts", ns.q[0].astype(np.float64), ns.k[0, :, 0].astype(np.float64)) * ns.scale * RM.LOG2E
        top = np.stack([s2[0][:, t * 64:(t + 1) * 64].max(-1) for t in range(c.Sk // 64)], -1)     # (rows, tiles)
        rise = np.diff(top, axis=-1).max(-1)
        for w0 in range(r0 + 32 - r0 % 32, r1 - 32, 32):
            assert (rise[w0:w0 + 32] > RM.K_THR).any() and (rise[w0:w0 + 32] < RM.K_THR).any(), (cid, w0)


# ---------------------------------------------------------------------------------------------------------------------
# mutants: the suite's own comparator must fail them
# ---------------------------------------------------------------------------------------------------------------------
PRESCALED_2X = ["offset-51nat", "offset-causal", "offset-heads1", "offset-heads2", "offset-cuts"]
PRESCALED_1X = ["offset-23nat", "offset-4ch"]


@pytest.mark.parametrize("cid", PRESCALED_2X + PRESCALED_1X)
def test_prescaled_k_model_fails_on_offset_inputs(cid):
    """The 64-row dK/dV kernel as it was (K * scale * log2(e) rounded to the 16-bit type once per item,
    `bwd_16bit_model(prescale_k=True)`).  Worst error / bound of the model, dk / dv:
        offset-51nat 2.71 / 2.52   offset-causal (= heads1, heads2) 5.37 / 4.75   offset-cuts 2.44 / 2.13
        offset-23nat 1.36 / 0.74   offset-4ch 1.51 / 1.20       (honest model on the same inputs: <= 0.11 / 0.01)
    At least 2x on the single-channel 51 nat instances.  The rounding error in the exponent is at most
    offset_log2 * 2^-9 per channel: 0.14 at 51 nat, 0.064 at 23 nat and per channel of the 4-channel spread -- a factor of
    at most 1.045 on a row, 0.9 x rtol: those two instances cannot reach 2x through rtol, the model fails them on dk by the
    margin recorded above (a kernel that rounds this way, on N(0,1) and needles: <= 0.5)."""
    r = _bwd(cid, prescale_k=True)
    if cid in PRESCALED_2X:
        assert r["dk"] >= 2.0 and r["dv"] >= 2.0, (cid, r)
    else:
        assert r["dk"] > 1.0, (cid, r)


SCALE_MUTANT_FAILS = ["offset-51nat", "offset-causal", "offset-d64-w32", "scale-1.0", "scale-0.3-w32", "pair-k-up"]


@pytest.mark.parametrize("cid", SCALE_MUTANT_FAILS)
def test_two_percent_scale_mutant_fails(cid):
    """softmax_scale * 1.02 in the kernel, the reference keeps the scale."""
    r = _bwd(cid, scale_mul=1.02)
    r.update(_fwd(cid, scale_mul=1.02)[0])
    assert max(r.values()) > 1.0, (cid, r)


def test_two_percent_scale_mutant_is_marginal_on_white_noise():
    """The expectation this family was proposed with -- that on N(0,1) with softmax_scale = D^-0.5 the 2 % mutant PASSES --
    does not hold: against the exact lse the model of that mutant misses every tensor there too (S 384, causal, bf16:
    out 1.32, lse 20.6, dq 1.50, dk 1.49, dv 2.07 x the bound).  What the value-range inputs add is margin: on white noise
    the mutant clears out and the gradients by at most 2.1x, within reach of a rounding change or another seed; on the
    offset inputs it misses dk and dv by 47 - 93x.  Both are asserted, so the point is on record as measured."""
    c = RI.Case("white", "scale", 384, 384, 4, 2, 128, True, "bfloat16", None, scale=128 ** -0.5)
    rs = np.random.RandomState(9)
    q, k, v, do = (round_to(x.astype(np.float32), c.dt) for x in RI._normals(c, rs))
    ns = RI._finish(c, q, k, v, do, c.scale)
    want = RI.reference(c, ns)
    out, lse, _ = RM.fwd_16bit_model(q, k, v, c.scale * 1.02, c.causal, c.dt)
    dq, dk, dv = RM.bwd_16bit_model(do, q, k, v, want["o16"], want["lse"], c.scale * 1.02, c.causal, c.dt, False)
    white = {n_: r for n_, (_, r) in RI.verdicts(c, ns, dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv), want).items()}
    assert all(white[n_] < 2.5 for n_ in ("out", "dq", "dk", "dv")), white
    sharp = _bwd("offset-51nat", scale_mul=1.02)
    assert sharp["dk"] > 20.0 and sharp["dv"] > 20.0 and sharp["dq"] > 5.0, sharp


@pytest.mark.parametrize("cid", ["scale-0.3", "scale-0.02-w32", "pair-q-up", "pair-k-down", "offset-51nat"])
def test_scale_missing_from_the_gradient_epilogue_fails(cid):
    """The scale applied inside P but not to dQ = scale dS K and dK = scale dS^T Q."""
    c, ns, _ = _case(cid)
    r = _bwd(cid, epilogue_div=ns.scale)
    assert r["dq"] > 1.0 and r["dk"] > 1.0 and r["dv"] <= 0.5, (cid, r)


NEVER_RAISED = [c.id for c in RI.STEPS if c.par[0] == "rise" and (c.dt == "float16" or c.par[1] == 40.0)]


@pytest.mark.parametrize("cid", NEVER_RAISED)
def test_forward_that_never_raises_its_reference_max_fails(cid):
    """P = exp2(S - max of the first tile), clamped to the 16-bit type's range: 2^16 is passed at the third tile of every
    fp16 series, 2^128 at the fifth tile of the bf16 series that rise by 40."""
    r, _ = _fwd(cid, raise_max=False)
    assert r["out"] > 1.0, (cid, r)


@pytest.mark.parametrize("cid", [c.id for c in RI.STEPS if c.par[0] == "fall" and c.dt == "float16"])
def test_forward_that_flushes_subnormal_p_fails(cid):
    """fp16: the second tile's aligned key weighs 2^-15 on the rows with multiplier 1.25 and carries v of 2^11."""
    r, _ = _fwd(cid, flush_subnormal=True)
    assert r["out"] > 1.0, (cid, r)
