"""Mutation tests: the GPU parity tests must be ABLE TO FAIL.

Every family of parity test (block kernels, packed mode, sliding window, K split / backward cuts, the virtual-rank
goldens, the sampled full-size checks) is run once more with the C-ABI binding patched so that, after the real
kernel has run, ONE element (or one whole row -- the image a NaN-prefilled buffer keeps when a kernel never writes
the row) of ONE result tensor is NaN.  The unmodified test function must then raise AssertionError.  A comparator
written as `bad = err > lim` passes all of these (NaN compares False); golden_util.assert_close does not.

The mutated position is (batch 0, LAST row, head 0, dim 0): every sampled test samples the last row / last key of
head 0, so the sampled families are covered by the same patch.
"""
import contextlib
import inspect

import numpy as np
import pytest
import torch

import test_gpu_parity as P
from golden_util import assert_close, close_mask

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import yunchang_amd  # noqa: F401
    from yunchang_amd import _C
    _C.load()
    return torch.device("cuda:0")


def _poison(t, kind):
    idx = (0,) * (t.dim() - 3) + (-1, 0)                  # (batch 0,) last row, head 0
    if kind == "elem":
        t[idx + (0,)] = float("nan")
    else:                                                 # "row": as if the kernel had never written the row
        t[idx] = float("nan")


@contextlib.contextmanager
def mutated(fn_name, arg_names, kind):
    """Patch yunchang_amd._C.<fn_name>: run the real launch, then poison the first result tensor among `arg_names`
    that the caller passed.  Yields a list that records the poisoned argument names (the test asserts it is
    non-empty: a mutation that never fired proves nothing)."""
    from yunchang_amd import _C
    real = getattr(_C, fn_name)
    sig = inspect.signature(real)
    fired = []

    def wrapper(*args, **kwargs):
        real(*args, **kwargs)
        bound = sig.bind(*args, **kwargs)
        for n in arg_names:
            t = bound.arguments.get(n)
            if t is not None:
                torch.cuda.current_stream().synchronize()
                _poison(t, kind)
                fired.append(n)
                break
    setattr(_C, fn_name, wrapper)
    try:
        yield fired
    finally:
        setattr(_C, fn_name, real)


FWD = ("flash_fwd", ("out", "acc"))
BWD_DQ = ("flash_bwd", ("dq16", "dq"))
BWD_DK = ("flash_bwd", ("dk16", "dk"))
BWD_DV = ("flash_bwd", ("dv16", "dv"))
PFWD = ("flash_fwd_packed", ("out", "acc"))
PBWD_DQ = ("flash_bwd_packed", ("dq16", "dq"))
PBWD_DV = ("flash_bwd_packed", ("dv16", "dv"))


def _must_fail(target, kind, fn, *args):
    with mutated(target[0], target[1], kind) as fired:
        with pytest.raises(AssertionError):
            fn(*args)
    assert fired, f"the mutation of {target} never fired in {fn.__name__}"


@pytest.mark.parametrize("kind", ["elem", "row"])
@pytest.mark.parametrize("target", [FWD, BWD_DQ, BWD_DK, BWD_DV], ids=["out", "dq", "dk", "dv"])
def test_block_family_fails_on_nan(dev, target, kind):
    _must_fail(target, kind, P.test_block_forward_backward_vs_oracle, dev, *P.SHAPES[1])
    _must_fail(target, kind, P.test_block_forward_backward_vs_oracle, dev, *P.SHAPES[3])      # ragged


@pytest.mark.parametrize("target,kind", [(FWD, "elem"), (FWD, "row"), (BWD_DQ, "elem"), (BWD_DK, "row"), (BWD_DV, "elem")],
                         ids=["out-elem", "out-row", "dq-elem", "dk-row", "dv-elem"])
def test_forced_row64_family_fails_on_nan(dev, target, kind):
    """The tests that pin the 64-row kernels (tests/test_gpu_row64.py) can fail too.  (Five of the eight (target, kind) pairs of
    round 5: each costs 5 s of oracle time in a suite with a time limit; both kinds stay covered on the forward and across the
    gradients.)"""
    import test_gpu_row64 as R
    _must_fail(target, kind, R.test_row64_edge_shapes, dev, *R.EDGE[4])          # ragged, bottom-right causal, GQA
    _must_fail(target, kind, R.test_row64_edge_shapes, dev, *R.EDGE[-1])         # several items per head
    if target is FWD:
        _must_fail(target, kind, R.test_row64_merge_in_and_partial_final_ranges, dev, *R.MERGE[1])


@pytest.mark.parametrize("target", [PFWD, PBWD_DQ, PBWD_DV], ids=["out", "dq", "dv"])
def test_packed_family_fails_on_nan(dev, target):
    _must_fail(target, "elem", P.test_packed_kernels_vs_oracle, dev, *P.PACKED[0])
    _must_fail(target, "row", P.test_packed_kernels_vs_oracle, dev, *P.PACKED[1])


@pytest.mark.parametrize("target", [FWD, BWD_DQ, BWD_DK], ids=["out", "dq", "dk"])
def test_window_family_fails_on_nan(dev, target):
    _must_fail(target, "elem", P.test_sliding_window_forward_backward_vs_oracle, dev, *P.WINDOWS[0])


def test_cut_families_fail_on_nan(dev):
    _must_fail(FWD, "elem", P.test_forward_k_split_through_the_binding, dev, 1, 1024, 1024, 2, 2, 128, True, "bfloat16")
    _must_fail(FWD, "row", P.test_forward_k_split_through_the_binding, dev, 1, 333, 200, 2, 1, 128, True, "bfloat16")
    for target in (BWD_DQ, BWD_DK, BWD_DV):
        _must_fail(target, "elem", P.test_backward_cuts_through_the_binding, dev, 1, 1024, 1024, 2, 2, 128, True,
                   "bfloat16")


@pytest.mark.parametrize("target", [FWD, BWD_DQ, BWD_DV], ids=["out", "dq", "dv"])
def test_virtual_rank_golden_family_fails_on_nan(dev, target):
    path = next(p for p in P.MULTI if P.Golden(p).bwd)
    _must_fail(target, "elem", P.test_multi_rank_golden_with_virtual_ranks, dev, path)


def test_varlen_golden_family_fails_on_nan(dev):
    from golden_util import varlen_golden_files
    _must_fail(PFWD, "elem", P.test_varlen_ring_golden_with_virtual_ranks, dev, varlen_golden_files()[0])


@pytest.mark.parametrize("target", [FWD, BWD_DQ, BWD_DK], ids=["out", "dq", "dk"])
def test_sampled_full_size_family_fails_on_nan(dev, target):
    """The NaN-prefilled buffers of this test were the reviewer's example: an unwritten row must not pass."""
    _must_fail(target, "row", P.test_c5_rank_block_shapes_against_sampled_fp64, dev, 16, 2)


def test_bench_sampled_parity_fails_on_nan(dev):
    """bench.sampled_parity (the 64K entry of the bench line): a NaN in a sampled row makes the figure NaN, and every
    gate written as `err < tol` is then False."""
    b = P._load_bench()
    t = b._fwd_bwd_kernels(1, 2048, 4, 2, 128, dev, 1, keep=True)["tensors"]
    clean = b.sampled_parity(t)["max_abs_err"]
    assert all(e == e for e in clean.values()) and clean["out"] < 2e-2 and clean["dq"] < 5e-2, clean
    for name in ("out", "dq", "dk", "dv"):
        u = dict(t)
        u[name] = t[name].clone()
        _poison(u[name], "elem")
        err = b.sampled_parity(u)["max_abs_err"]
        assert err[name] != err[name], (name, err)                       # NaN
        assert not (err[name] < 1.0)


@pytest.mark.parametrize("target,kind", [(FWD, "elem"), (FWD, "row"), (BWD_DQ, "row"), (BWD_DK, "elem"), (BWD_DV, "row")],
                         ids=["out-elem", "out-row", "dq-row", "dk-elem", "dv-row"])
def test_large_launch_family_fails_on_nan(dev, target, kind):
    """The every-element checks at multi-pass launch sizes (tests/test_gpu_large_launch.py) can fail (case J: the cheapest
    reference of the table)."""
    import test_gpu_large_launch as LL
    _must_fail(target, kind, LL.run_case, dev, LL._BY_ID["J"])


@contextlib.contextmanager
def copied_head_block(fn_name, arg_names):
    """Patch yunchang_amd._C.<fn_name>: after the real launch, copy a 64-row block of head 1 over head 0 in the middle of
    the sequence of the first result tensor among `arg_names` -- finite values, the image of an item walk that ran the wrong
    head."""
    from yunchang_amd import _C
    real = getattr(_C, fn_name)
    sig = inspect.signature(real)
    fired = []

    def wrapper(*args, **kwargs):
        real(*args, **kwargs)
        bound = sig.bind(*args, **kwargs)
        for n in arg_names:
            t = bound.arguments.get(n)
            if t is not None:
                torch.cuda.current_stream().synchronize()
                mid = t.shape[1] // 2
                t[:, mid:mid + 64, 0] = t[:, mid:mid + 64, 1]
                fired.append(n)
                break
    setattr(_C, fn_name, wrapper)
    try:
        yield fired
    finally:
        setattr(_C, fn_name, real)


@pytest.mark.parametrize("target", [FWD, BWD_DQ], ids=["out", "dq"])
def test_large_launch_family_fails_on_a_wrong_head(dev, target):
    import test_gpu_large_launch as LL
    with copied_head_block(*target) as fired:
        with pytest.raises(AssertionError):
            LL.run_case(dev, LL._BY_ID["J"])
    assert fired, f"the mutation of {target} never fired"


@pytest.mark.parametrize("kind", ["nan", "head"])
@pytest.mark.parametrize("target", ["out", "dq", "dk", "dv"])
def test_layout_family_fails_on_an_injection_into_the_strided_run(dev, target, kind):
    """The layout sweeps (tests/test_gpu_layouts.py) run every case contiguous and strided and compare the bits.  Here the
    STRIDED run's result gets one NaN (a computed one, not the arena's sentinel: the "was it written" checks pass) or a
    64-row block of head 1 copied over head 0 after the real launch: the unmodified runner must fail, in its bit comparison."""
    import layout_util as LU
    import test_gpu_layouts as G

    class Injected(G.HipOps):
        """The second flash call of the runner is the strided one."""
        calls = fired = 0

        def _inject(self, t):
            self.calls += 1
            if self.calls != 2:
                return
            torch.cuda.synchronize()
            if kind == "nan":
                t[0, -1, 0, 0] = float("nan")
            else:
                mid = t.shape[1] // 2
                t[:, mid:mid + 64, 0] = t[:, mid:mid + 64, 1]
            self.fired += 1

        def fwd(self, q, k, v, scale, causal, lse, out=None, **kw):
            G.HipOps.fwd(self, q, k, v, scale, causal, lse, out=out, **kw)
            self._inject(out)

        def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, *a, **kw):
            G.HipOps.bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, *a, **kw)
            self._inject({"dq": kw["dq16"], "dk": kw["dk16"], "dv": kw["dv16"]}[target])

    case = LU.Case(2, 200, 260, 4, 2, 64, True, "bfloat16", family="wave32")
    check = LU.check_fwd_case if target == "out" else LU.check_bwd_case
    check(G.HipOps(), case, 5, dev)                            # the case itself passes
    ops = Injected()
    with pytest.raises(AssertionError, match="differ in their bits"):
        check(ops, case, 5, dev)
    assert ops.fired == 1, "the injection never fired"


# ------------------------------------------------------------------------------------------------
# needle inputs (tests/test_gpu_needle.py): the REAL kernel on altered operands -- finite, plausible, subtly wrong results
# ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def altered(fn_name, alter):
    """Patch yunchang_amd._C.<fn_name>: `alter(arguments)` edits the bound arguments (a dict; tensors must be replaced by
    altered COPIES, never written to), then the real launch runs on them.  Yields the list of the calls it altered."""
    from yunchang_amd import _C
    real = getattr(_C, fn_name)
    sig = inspect.signature(real)
    fired = []

    def wrapper(*args, **kwargs):
        bound = sig.bind(*args, **kwargs)
        alter(bound.arguments)
        fired.append(fn_name)
        return real(*bound.args, **bound.kwargs)
    setattr(_C, fn_name, wrapper)
    try:
        yield fired
    finally:
        setattr(_C, fn_name, real)


def _zero_keys(k0, k1):
    def alter(a):
        k = a["k"].clone()
        k[:, k0:k1] = 0
        a["k"] = k
    return alter


def _swap_key_tiles(t):
    def alter(a):
        k = a["k"].clone()
        k[:, t:t + 64], k[:, t + 64:t + 128] = a["k"][:, t + 64:t + 128], a["k"][:, t:t + 64]
        a["k"] = k                                          # (V is left alone: K tile t meets V tile t + 1)
    return alter


def _window_left_off_by_one(a):
    a["window"] = (a["window"][0] + 1, a["window"][1])


def _swap_dout_heads(a):
    do = a["dout"].clone()
    do[:, 256:512, 0], do[:, 256:512, 1] = a["dout"][:, 256:512, 1], a["dout"][:, 256:512, 0]
    a["dout"] = do                                          # (heads 0 and 1 share a KV group)


def _needle_must_fail(dev, fn_name, alter, cfg_id):
    import test_gpu_needle as GN
    c = GN._CFG[cfg_id]
    GN.run_dense(dev, c)                                    # the case itself passes
    with altered(fn_name, alter) as fired:
        with pytest.raises(AssertionError, match="out of tolerance"):
            GN.run_dense(dev, c)
    assert fired, f"the alteration of {fn_name} never fired in {cfg_id}"


@pytest.mark.parametrize("fn_name", ["flash_fwd", "flash_bwd"])
@pytest.mark.parametrize("cfg_id", ["row64-causal", "wave4-d128"])
def test_needle_family_fails_on_a_zeroed_key_tile(dev, cfg_id, fn_name):
    """The 64-key tile [128, 192) of K reads as zeros (the image of a tile the kernel never loaded): every result stays
    finite and on N(0,1) inputs within tolerance at depth; the needle test must fail, forward and backward."""
    _needle_must_fail(dev, fn_name, _zero_keys(128, 192), cfg_id)


@pytest.mark.parametrize("fn_name", ["flash_fwd", "flash_bwd"])
def test_needle_family_fails_on_swapped_key_tiles(dev, fn_name):
    """K tiles [256, 320) and [320, 384) swapped, V left alone: every key is counted once, with the neighbour's V."""
    _needle_must_fail(dev, fn_name, _swap_key_tiles(256), "row64-causal")


@pytest.mark.parametrize("fn_name", ["flash_fwd", "flash_bwd"])
def test_needle_family_fails_on_a_window_left_bound_off_by_one(dev, fn_name):
    _needle_must_fail(dev, fn_name, _window_left_off_by_one, "win-causal")


def test_needle_family_fails_on_a_zeroed_key_at_a_k_split_run_boundary(dev):
    """The first key of the second of the three runs the LAST query tile's keys are cut into reads as zeros."""
    import needle_inputs as NI
    import test_gpu_needle as GN
    c = GN._CFG["ksplit3-row64"]
    q0 = (c.Sq - 1) // 256 * 256
    t0, nt = NI.key_tiles_of_query_tile(q0, 256, c.Sq, c.Sk, c.causal)
    kb = NI.run_bounds(t0, nt, c.k_splits, "floor")[0] * 64
    _needle_must_fail(dev, "flash_fwd", _zero_keys(kb, kb + 1), "ksplit3-row64")


def test_needle_family_fails_on_dout_heads_swapped_inside_a_gqa_group(dev):
    _needle_must_fail(dev, "flash_bwd", _swap_dout_heads, "gqa8-heads2")


def _shift_plus(d):
    def alter(a):
        a["shift"] = a["shift"] + d
    return alter


def _window_right_off_by_one(a):
    a["window"] = (a["window"][0], a["window"][1] + 1)


_SHIFT_ALTERED = [("sh-r64-causal+70", "shift+1", _shift_plus(1)), ("sh-r64-causal+70", "shift-1", _shift_plus(-1)),
                  ("sh-r64-right-70", "right+1", _window_right_off_by_one),
                  ("sh-w4-both-100", "shift+1", _shift_plus(1)), ("sh-w4-both-100", "shift-1", _shift_plus(-1)),
                  ("sh-w4-both-100", "left+1", _window_left_off_by_one)]


@pytest.mark.parametrize("fn_name", ["flash_fwd", "flash_bwd"])
@pytest.mark.parametrize("cfg_id,alter", [(c, f) for c, _, f in _SHIFT_ALTERED], ids=[f"{c}:{n}" for c, n, _ in _SHIFT_ALTERED])
def test_shifted_needle_family_fails_on_a_bound_one_key_off(dev, cfg_id, alter, fn_name):
    """The REAL kernel is handed shift + 1, shift - 1, or a window bound + 1 with the shift unchanged: one key more or less on
    one bound of every row -- a few 1e-3 of `out` on N(0,1) inputs at these depths.  The shifted needle cases (64-row: causal +
    shift; 32-row: both bounds + shift) must fail, forward and backward.  (A causal case has no window to move and the 64-row
    family serves no left bound that cuts: its third alteration is the RIGHT bound + 1 of `sh-r64-right-70`.)"""
    _needle_must_fail(dev, fn_name, alter, cfg_id)


# ------------------------------------------------------------------------------------------------
# value-range inputs (tests/test_gpu_range.py): the REAL kernel is handed softmax_scale * 1.02, the reference keeps the scale
# ------------------------------------------------------------------------------------------------
def _scale_times_1_02(a):
    a["softmax_scale"] = a["softmax_scale"] * 1.02


@pytest.mark.parametrize("fn_name", ["flash_fwd", "flash_bwd"])
@pytest.mark.parametrize("cid", ["offset-causal", "scale-0.3-w32"])
def test_range_family_fails_on_a_scale_two_percent_off(dev, cid, fn_name):
    import test_gpu_range as GR
    run = GR.run_forward if fn_name == "flash_fwd" else GR.run_backward
    run(dev, cid)                                           # the case itself passes
    with altered(fn_name, _scale_times_1_02) as fired:
        with pytest.raises(AssertionError, match="out of tolerance"):
            run(dev, cid)
    assert fired, f"the alteration of {fn_name} never fired in {cid}"


def test_comparator_itself():
    """The comparator on host arrays (also covered without a GPU by tests/test_oracle_golden.py)."""
    want = np.array([1.0, -np.inf, 2.0])
    assert_close(np.array([1.0, -np.inf, 2.0]), want, 1e-3, 0, "same -inf passes")
    for got in ([np.nan, -np.inf, 2.0], [1.0, np.inf, 2.0], [1.0, np.nan, 2.0], [1.0, -np.inf, 3.0]):
        ok, _ = close_mask(np.array(got), want, 1e-3, 0)
        assert not ok.all()
        with pytest.raises(AssertionError):
            assert_close(np.array(got), want, 1e-3, 0)
