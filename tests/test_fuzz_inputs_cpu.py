"""The inputs of tests/test_gpu_fuzz_sink_doc.py can fail: with the fp64 references alone (tests/doc_ref.py, tests/sink_ref.py), on
the first 12 seeds of each GPU sweep, drawn by the GPU file's own functions and judged at its tolerances (doc_tol, sink_tol), a
reference that is wrong by ONE step fails the comparison the GPU test makes.

Document mask: every single-step change of a launch's arrays (tests/stair_inputs.py: launch_mutants -- a boundary of a list
moved by one position, a plateau's bound moved by one key, a plateau edge moved by one row) that changes the mask fails `out` and
`dv`, and `dq` and `dk` too unless every row whose visible set it changes sees at most one key in the true or in the changed mask
(one visible key: P = 1, dS = 0 by arithmetic, whatever the key).  Sinks: a missing sink, a sink counted twice and sinks read for
the neighbouring head fail `lse`; missing and rolled fail `out` as well.  These are conditions on the inputs, not measurements:
each case prints what it judged."""
import math

import numpy as np
import pytest
import torch

import doc_ref
import needle_inputs
import sink_ref
import stair_inputs as SI
from test_gpu_fuzz_sink_doc import doc_case, doc_inputs, doc_tol, redraw_cap_holds, sink_case, sink_inputs, sink_tol

SEEDS = range(12)


def _fails(got, want, tol):
    ok, ratio = needle_inputs.bound_ratio(got.numpy(), want.numpy(), *tol)
    return (not ok), ratio


@pytest.mark.parametrize("seed", SEEDS)
def test_doc_mutants_fail(seed):
    c = doc_case(seed)
    la, B, Sq, Sk, G, dt = c.launch, c.B, c.Sq, c.Sk, c.G, c.dt
    nd = doc_inputs(c)
    q, k, v, do = (torch.from_numpy(x.astype(np.float32)).to(getattr(torch, dt)) for x in (nd.q, nd.k, nd.v, nd.do))
    scale = c.D ** -0.5
    mask = doc_ref.block_mask(la.row_lo, Sq, Sk, la.causal, B)
    true = dict(zip(("out", "lse", "dq", "dk", "dv"), doc_ref.ref_bwd(do, q, k, v, scale, mask, out_dtype=q.dtype)))
    tol = {n: doc_tol(n, dt, G, Sq, Sk, true[n]) for n in ("out", "dq", "dk", "dv")}       # of the whole launch, as the GPU test has them
    muts, same = SI.launch_mutants(la)
    judged = exceptions = undetected = 0
    worst = float("inf")
    for name, b, rl in muts:
        e = slice(b, b + 1)                                      # (a shared array: entry 0 stands for the batch)
        m = doc_ref.block_mask(rl, Sq, Sk, la.causal)
        changed = (m != mask[e]).any(-1)[0]
        assert bool(changed.any()), name
        seen = torch.minimum(m[0].sum(-1), mask[b].sum(-1))[changed]
        one_key = bool((seen <= 1).all())
        wrong = dict(zip(("out", "lse", "dq", "dk", "dv"), doc_ref.ref_bwd(do[e], q[e], k[e], v[e], scale, m, out_dtype=q.dtype)))
        res = {n: _fails(wrong[n], true[n][e], tol[n]) for n in tol}
        judged += 1
        undetected += not any(f for f, _ in res.values())
        for n in ("out", "dv"):
            assert res[n][0], f"{c.what}: {name} passes in {n} (worst err / bound {res[n][1]:.2f})"
        if one_key and not (res["dq"][0] and res["dk"][0]):
            exceptions += 1
        else:
            for n in ("dq", "dk"):
                assert res[n][0], f"{c.what}: {name} passes in {n} (worst err / bound {res[n][1]:.2f})"
            worst = min(worst, min(r for _, r in res.values()))
    print(f"[fuzz-inputs] {c.what}: mutants judged {judged} / exceptions (one visible key: dS = 0) {exceptions} / undetected "
          f"{undetected} / dropped, mask unchanged {same} / smallest err : bound of a failing tensor {worst:.1f}")
    assert judged == len(muts) and judged >= 1 and undetected == 0, (c.what, judged, len(muts), undetected)


def test_doc_draws_cover_what_they_must():
    """Over the default sweep: both kinds of list launch and staircases, shared arrays and arrays per entry, Sq != Sk, a run of
    documents of length 1, and -- with B > 1 -- an entry that sees nothing beside one that does."""
    from test_gpu_fuzz_sink_doc import _N_DOC
    cases = [doc_case(s) for s in range(max(_N_DOC, 24))]
    kinds = {c.launch.kind for c in cases}
    assert kinds == {"whole", "block", "stairs"}, kinds
    assert any(c.launch.shared and c.B > 1 for c in cases) and any(not c.launch.shared for c in cases)
    assert any(c.Sq != c.Sk for c in cases if c.launch.kind == "block") and any(c.Sq != c.Sk for c in cases if c.launch.kind == "stairs")
    assert any(any(e) and not all(e) for c in cases for e in [c.launch.empty] if c.launch.kind == "block")
    assert any(1 in np.diff(cu).tolist()[1:] and (np.diff(cu) == 1).sum() >= 6 for c in cases if c.launch.kind == "whole" for cu in c.launch.lists)
    assert any(c.ring for c in cases) and any(c.cut for c in cases) and any(c.only for c in cases)
    for c in cases:                                              # what the ABI asks of the arrays
        rl, kh = np.asarray(c.launch.row_lo).reshape(-1, c.Sq), np.asarray(c.launch.key_hi).reshape(-1, c.Sk)
        assert rl.dtype == np.int32 and kh.dtype == np.int32 and len(rl) == len(kh) == (1 if c.launch.shared else c.B)
        for r, h in zip(rl, kh):
            assert (np.diff(r) >= 0).all() and (np.diff(h) >= 0).all() and 0 <= r.min() and r.max() <= c.Sk and 0 <= h.min() and h.max() <= c.Sq
            assert np.array_equal(h, SI.key_hi_of(r, c.Sk)), c.what


@pytest.mark.parametrize("seed", SEEDS)
def test_sink_mutants_fail(seed):
    c = sink_case(seed)
    (q, k, v, do, s), ref, _ = sink_inputs(c, "cpu")
    scale = c.D ** -0.5
    muts = {"missing": torch.full_like(s, -1e4), "twice": s + math.log(2.0)}
    if c.Hq > 1:
        muts["rolled"] = torch.roll(s, 1)
    sees = bool(sink_ref.alibi_ref.visible(c.Sq, c.Sk, c.causal, c.win, c.shift, "cpu").any())
    rep = {}
    for name, m in muts.items():
        w = sink_ref.ref_fwd(q, k, v, scale, m, c.causal, c.win, c.shift)
        res = {n: _fails(w[i], ref[i], sink_tol(n, c.dt, c.G, c.Sq, c.Sk, ref[i])) for i, n in enumerate(("out", "lse"))}
        rep[name] = {n: round(r, 1) for n, (_, r) in res.items()}
        assert res["lse"][0], f"{c.what}: sinks {name} pass in lse (worst err / bound {res['lse'][1]:.2f})"
        if name != "twice":
            # (a launch in which no row sees a key has out = 0 whatever the sinks: the lse alone carries them there)
            assert res["out"][0] or not sees, f"{c.what}: sinks {name} pass in out (worst err / bound {res['out'][1]:.2f})"
    print(f"[fuzz-inputs] {c.what}: a row sees a key: {sees}; worst err : bound of the mutants {rep}")


def test_sink_redraws_stay_rare():
    """Over the default sweep no case is dropped and at most one in six draws v / dout again."""
    from test_gpu_fuzz_sink_doc import _N_SINKS, _REDRAWS
    for seed in range(max(_N_SINKS, 18)):
        if seed not in _REDRAWS:
            sink_inputs(sink_case(seed), "cpu")
    print(f"[fuzz-inputs] further draws of v / dout per seed: {dict(sorted(_REDRAWS.items()))}")
    assert redraw_cap_holds(), _REDRAWS
