"""The layout harness (tests/layout_util.py) proves itself without a GPU.

The case runners that tests/test_gpu_layouts.py drives against the HIP kernels run here against the CPU oracle backend
(tests/oracle_backend.py) and must pass; against deliberately wrong wrappers of it -- one per stride triple / pair of the
forward, delta and backward argument blocks, each addressing ONE tensor through another tensor's strides -- they must fail.
That also pins the generator: two tensors whose drawn layouts coincided at every seed would leave the sweep blind to that
mix-up, and the mutant would survive."""
import numpy as np
import pytest
import torch

import layout_util as LU
from oracle_backend import OracleBlockBackend

N_SEEDS = 10
DEV = torch.device("cpu")


class OracleOps:
    """The runner's `ops` seam over the CPU oracle backend (no kernel families, no softcap: launch-only arguments drop)."""

    def __init__(self):
        self.be = OracleBlockBackend()

    def fwd(self, q, k, v, scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None, k_splits=0,
            window=None, softcap=None, family=None):
        assert not softcap
        self.be.fwd(q, k, v, scale, causal, lse, out=out, acc=acc, merge_in=merge_in, final_begin=final_begin,
                    final_end=final_end, window=window, k_splits=k_splits)

    def delta(self, dout, out, delta):
        self.be.delta(dout, out, delta)

    def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, scale, causal, accum_dq=False, accum_dk=False, accum_dv=False,
            dq16=None, dk16=None, dv16=None, window=None, softcap=None, family=None, only=None, splits=None, dkdv_heads=0):
        assert not softcap
        self.be.bwd(dout, q, k, v, lse, delta, dq, dk, dv, scale, causal, accum_dq, accum_dk, accum_dv, dq16, dk16, dv16,
                    window=window, only=only)

    def fwd_packed(self, q, k, v, seq_q, seq_k, max_q, max_k, scale, causal, lse, out=None, sched=True, softcap=None):
        assert not softcap
        self.be.fwd_packed(q, k, v, seq_q, seq_k, max_q, max_k, scale, causal, lse, out=out)

    def bwd_packed(self, dout, q, k, v, lse, delta, seq_q, seq_k, max_q, max_k, dq, dk, dv, scale, causal, accum_dq=False,
                   accum_dk=False, accum_dv=False, dq16=None, dk16=None, dv16=None, sched=True, softcap=None):
        assert not softcap
        self.be.bwd_packed(dout, q, k, v, lse, delta, seq_q, seq_k, max_q, max_k, dq, dk, dv, scale, causal, accum_dq, accum_dk,
                           accum_dv, dq16, dk16, dv16)

    def kinds(self):
        return None


def small_case(rs, call):
    """Small ragged shapes (the fp64 oracle runs dozens of times per mutant): Sq != Sk, GQA, B up to 3, both dtypes."""
    if call == "packed":
        return LU.draw_packed_case(rs, 0, 40, (32, 64))
    D = int(rs.choice([32, 64]))
    dt = str(rs.choice(["bfloat16", "float16"]))
    Hkv = int(rs.choice([1, 2]))
    Hq = Hkv * int(rs.choice([1, 2]))
    B = int(rs.choice([1, 2, 2, 3]))
    Sq, Sk = int(rs.randint(3, 60)), int(rs.randint(3, 60))
    causal = bool(rs.rand() < 0.5)
    kw = {}
    if call == "fwd" and rs.rand() < 0.5:
        Sa = int(rs.randint(1, Sk)) if Sk > 1 else 0
        fb = int(rs.randint(0, Sq))
        kw["ring"] = (Sa, fb, int(rs.randint(fb, Sq + 1)))
    if call == "bwd":
        kw["forms"] = tuple(str(rs.choice(["f32", "f32+", "h16", "h16+"])) for _ in range(3))
        kw["only"] = [None, None, "dq", "dkdv"][rs.randint(4)]
    return LU.Case(B, Sq, Sk, Hq, Hkv, D, causal, dt, **kw)


CHECK = {"fwd": LU.check_fwd_case, "bwd": LU.check_bwd_case, "delta": LU.check_delta_case, "packed": LU.check_packed_case}


@pytest.mark.parametrize("call", ["fwd", "delta", "bwd", "packed"])
def test_runner_passes_on_the_oracle_backend(call):
    for seed in range(N_SEEDS):
        CHECK[call](OracleOps(), small_case(np.random.RandomState(300 + seed), call), seed, DEV)


# ---- wrong backends ------------------------------------------------------------------------------------------------------
class Escaped(AssertionError):
    """The wrongly strided view does not even fit the slab: on a device that is a read / write outside the arena."""


def _through(t, other, dims=(0, 1, 2)):
    """`t`'s pointer and shape with `other`'s strides in `dims` (other: a tensor, or "contig")."""
    if t is None:
        return None
    want = list(t.stride())
    src = torch.empty(t.shape).stride() if isinstance(other, str) else other.stride()
    for d in dims:
        if d < t.dim() - 1 and t.shape[d] > 1:            # (the stride of a dimension of size 1 addresses nothing)
            want[d] = src[d]
    if want == list(t.stride()):
        return t
    try:
        return t.as_strided(t.shape, want, t.storage_offset())
    except RuntimeError as e:
        raise Escaped(str(e)) from None


class Mixup(OracleOps):
    """Addresses tensor `target` of call `call` through the strides of `source` (same call; "contig" = as if it were
    contiguous).  `fired` counts the calls in which that changed the view."""

    def __init__(self, call, target, source, dims=(0, 1, 2)):
        super().__init__()
        self.call, self.target, self.source, self.dims, self.fired = call, target, source, dims, 0

    def _mix(self, names, args, unused=()):
        a = dict(zip(names, args))
        t = a.get(self.target)                                 # (None: not a tensor of this call of the sequence)
        if t is not None and self.target not in unused:        # (a tensor the call does not touch may have any strides)
            src = self.source if self.source == "contig" else a[self.source]
            if src is not None:
                m = _through(t, src, self.dims)
                self.fired += m is not t
                a[self.target] = m
        return [a[n] for n in names]

    def fwd(self, q, k, v, scale, causal, lse, out=None, acc=None, **kw):
        if self.call == "fwd":
            fe = q.shape[1] if kw.get("final_end") is None else kw["final_end"]
            unused = ("out",) if fe <= kw.get("final_begin", 0) else ()
            q, k, v, lse, out, acc = self._mix(("q", "k", "v", "lse", "out", "acc"), (q, k, v, lse, out, acc), unused)
        super().fwd(q, k, v, scale, causal, lse, out=out, acc=acc, **kw)

    def delta(self, dout, out, delta):
        if self.call == "delta":
            dout, out, delta = self._mix(("dout", "o", "delta"), (dout, out, delta))
        super().delta(dout, out, delta)

    def fwd_packed(self, q, k, v, seq_q, seq_k, max_q, max_k, scale, causal, lse, out=None, **kw):
        if self.call == "packed":
            q, k, v, lse, out = self._mix(("q", "k", "v", "lse", "out"), (q, k, v, lse, out))
        super().fwd_packed(q, k, v, seq_q, seq_k, max_q, max_k, scale, causal, lse, out=out, **kw)

    def bwd_packed(self, dout, q, k, v, lse, delta, seq_q, seq_k, max_q, max_k, dq, dk, dv, scale, causal, accum_dq=False,
                   accum_dk=False, accum_dv=False, dq16=None, dk16=None, dv16=None, **kw):
        if self.call == "packed":
            names = ("dout", "q", "k", "v", "lse", "delta", "dq", "dk", "dv", "dq16", "dk16", "dv16")
            dout, q, k, v, lse, delta, dq, dk, dv, dq16, dk16, dv16 = self._mix(
                names, (dout, q, k, v, lse, delta, dq, dk, dv, dq16, dk16, dv16))
        super().bwd_packed(dout, q, k, v, lse, delta, seq_q, seq_k, max_q, max_k, dq, dk, dv, scale, causal, accum_dq, accum_dk,
                           accum_dv, dq16, dk16, dv16, **kw)

    def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, scale, causal, accum_dq=False, accum_dk=False, accum_dv=False,
            dq16=None, dk16=None, dv16=None, **kw):
        if self.call == "bwd":
            names = ("dout", "q", "k", "v", "lse", "delta", "dq", "dk", "dv", "dq16", "dk16", "dv16")
            unused = {None: (), "dq": ("dk", "dv", "dk16", "dv16"), "dkdv": ("dq", "dq16")}[kw.get("only")]
            dout, q, k, v, lse, delta, dq, dk, dv, dq16, dk16, dv16 = self._mix(
                names, (dout, q, k, v, lse, delta, dq, dk, dv, dq16, dk16, dv16), unused)
        super().bwd(dout, q, k, v, lse, delta, dq, dk, dv, scale, causal, accum_dq, accum_dk, accum_dv, dq16, dk16, dv16, **kw)


class StorePastPaddedRow(OracleOps):
    """After the forward, one store 8 elements past the end of the first row of `out` when that row is padded."""

    def __init__(self):
        super().__init__()
        self.fired = 0

    def fwd(self, q, k, v, scale, causal, lse, out=None, acc=None, **kw):
        super().fwd(q, k, v, scale, causal, lse, out=out, acc=acc, **kw)
        D = q.shape[3]
        if out is not None and min(out.stride(2), out.stride(1)) >= D + 9:
            out.as_strided((1,), (1,), out.storage_offset() + D + 7).fill_(1.0)
            self.fired += 1


class WritesNonFinalRow(OracleOps):
    """A forward that also stores a row of `out` outside [final_begin, final_end)."""

    def __init__(self):
        super().__init__()
        self.fired = 0

    def fwd(self, q, k, v, scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None, **kw):
        super().fwd(q, k, v, scale, causal, lse, out=out, acc=acc, merge_in=merge_in, final_begin=final_begin,
                    final_end=final_end, **kw)
        Sq = q.shape[1]
        fe = Sq if final_end is None else final_end
        if out is not None and fe > final_begin and (final_begin > 0 or fe < Sq):
            out[:, 0 if final_begin > 0 else Sq - 1] = 0.5
            self.fired += 1


MUTANTS = [
    # (call, target, source, dims)   -- one per stride triple / pair of the argument blocks
    ("fwd", "q", "k", (0, 1, 2)), ("fwd", "k", "v", (0, 1, 2)), ("fwd", "v", "k", (0, 1, 2)),
    ("fwd", "out", "acc", (0, 1, 2)), ("fwd", "acc", "out", (0, 1, 2)), ("fwd", "lse", "contig", (0, 1)),
    ("delta", "dout", "o", (0, 1, 2)), ("delta", "o", "dout", (0, 1, 2)), ("delta", "delta", "contig", (0, 1)),
    ("bwd", "dout", "q", (0,)),                              # dout through q's BATCH stride only
    ("bwd", "dout", "q", (0, 1, 2)), ("bwd", "q", "dout", (0, 1, 2)), ("bwd", "k", "v", (0, 1, 2)), ("bwd", "v", "k", (0, 1, 2)),
    ("bwd", "dq", "contig", (0, 1, 2)), ("bwd", "dk", "dv", (0, 1, 2)), ("bwd", "dv", "dk", (0, 1, 2)),
    ("bwd", "dq16", "contig", (0, 1, 2)), ("bwd", "dk16", "dv16", (0, 1, 2)), ("bwd", "dv16", "dk16", (0, 1, 2)),
    ("bwd", "lse", "delta", (0, 1)), ("bwd", "delta", "lse", (0, 1)),
    # packed mode: token tensors (stride_s, stride_h) and (H,T) row statistics (stride_h)
    ("packed", "v", "k", (0, 1)), ("packed", "out", "contig", (0, 1)), ("packed", "dout", "q", (0, 1)), ("packed", "dk16", "dv16", (0, 1)),
    ("packed", "dv", "dk", (0, 1)), ("packed", "delta", "lse", (0,)),
]


NAMES = {"fwd": LU.FWD_TENSORS, "bwd": LU.BWD_TENSORS, "delta": LU.DELTA_TENSORS, "packed": LU.PACKED_TENSORS}


def _sweep(make_ops, call, n=3 * N_SEEDS, fixed=None):
    """Run the sweep against fresh wrong backends: (cases in which the mutation changed a view, cases caught by the
    comparators, cases whose wrong view left the slab)."""
    fired = caught = escaped = 0
    for seed in range(n):
        ops = make_ops()
        case = small_case(np.random.RandomState(300 + seed), call)
        layouts = None
        if fixed:
            layouts = dict(LU.draw_layouts(np.random.RandomState(90000 + seed), case, NAMES[call], seed), **fixed)
        try:
            CHECK[call](ops, case, seed, DEV, layouts)
        except Escaped:
            escaped += 1
            fired += 1
            continue
        except AssertionError:
            assert ops.fired, "the runner failed although the backend did nothing wrong"
            caught += 1
        fired += bool(ops.fired)
    return fired, caught, escaped


@pytest.mark.parametrize("call,target,source,dims", MUTANTS, ids=[f"{c}-{t}-via-{s}-{len(d)}" for c, t, s, d in MUTANTS])
def test_runner_catches_a_tensor_addressed_through_other_strides(call, target, source, dims):
    fired, caught, escaped = _sweep(lambda: Mixup(call, target, source, dims), call)
    assert fired >= 5, f"the drawn layouts of {target} and {source} differ in only {fired} cases: the generator is blind here"
    assert caught >= 1, "no case was caught by the comparators themselves"
    # EVERY case in which the wrong strides address other memory must be noticed
    assert caught + escaped == fired, f"{fired - caught - escaped} of {fired} wrong runs passed"


def test_runner_catches_a_store_past_a_padded_row():
    fired, caught, _ = _sweep(StorePastPaddedRow, "fwd", N_SEEDS, fixed=dict(out=LU.Layout("row_pad", "out16", pad=3)))
    assert fired >= 3 and caught == fired, (fired, caught)


def test_runner_catches_a_write_to_a_non_final_row():
    fired, caught, _ = _sweep(WritesNonFinalRow, "fwd")
    assert fired >= 3 and caught == fired, (fired, caught)


# ---- place / draw_layout ---------------------------------------------------------------------------------------------------
ELEM = {torch.bfloat16: 2, torch.float16: 2, torch.float32: 4}


@pytest.mark.parametrize("role,dtype", [("in16", torch.bfloat16), ("in16", torch.float16), ("f32", torch.float32),
                                        ("out16", torch.float16), ("lse", torch.float32)])
def test_place_alignment_coverage_and_disjoint_views(role, dtype):
    seen = {1: set(), 2: set()}
    for seed in range(240):
        rs = np.random.RandomState(seed)
        B = 1 + seed % 2 * int(rs.randint(1, 3))
        S, H, D = int(rs.randint(1, 40)), int(rs.randint(1, 5)), int(rs.choice([32, 64, 128]))
        L = LU.draw_layout(rs, role, B)
        seen[min(B, 2)].add(L.kind)
        ar = LU.Arena(DEV)
        shape = (B, H, S) if role == "lse" else (B, S, H, D)
        x = torch.randn(shape).to(dtype)
        v = LU.place(x, L, ar, "x", ss_mult=128 if (role == "in16" and seed % 3 == 0) else 1)
        assert torch.equal(v, x) and ar.unchanged(v) and ar.untouched(), L
        assert v.stride(-1) == 1
        ptr_align, stride_align = {"in16": (16, 8), "f32": (16, 4), "out16": (8, 4), "lse": (4, 1)}[role]
        assert v.data_ptr() % ptr_align == 0, (L, v.data_ptr())
        for d in range(v.dim() - 1):
            assert v.stride(d) % stride_align == 0, (L, v.stride())
        if role == "in16" and seed % 3 == 0:
            assert v.stride(1) % 128 == 0, (L, v.stride())
        if L.kind == "base8":
            assert v.data_ptr() % 16 == 8
        if L.kind == "stride4":
            assert all(s % 8 == 4 for s in v.stride()[(1 if B == 1 else 0):3]), v.stride()
        if L.kind == "base4":
            assert v.data_ptr() % 8 == 4
        rows = v.shape[1] * v.stride(1) * ELEM[dtype]
        assert rows < 2 ** 27                                # far below the 32-bit offsets of the kernels
        # no two elements of the view share an address, all of them lie inside the slab's data area
        _, raw, owned, _ = ar.slabs[0]
        assert int(owned.sum()) == x.numel(), L
        assert not bool(owned[:ar.FRONT].any()) and not bool(owned[-ar.BACK:].any())
        # a store just outside the view is seen
        raw[ar.FRONT - 1] = 0
        assert not ar.untouched()
        # ... and so is a modified input
        v[(0,) * v.dim()] += 1.0
        assert not ar.unchanged(v)
    want = set(LU.kinds_for(role, 2))
    assert seen[2] >= want, f"{role}: kinds never drawn at B > 1: {want - seen[2]}"
    assert seen[1] >= set(LU.kinds_for(role, 1)), f"{role}: kinds never drawn at B == 1: {set(LU.kinds_for(role, 1)) - seen[1]}"


def test_every_kind_occurs_for_every_tensor_within_the_default_seed_count():
    """Over the cases the GPU sweep draws at its default count (the generators are host code), every tensor of the forward
    and of the backward call sees every layout kind of its role, and every role the two B == 1 kinds."""
    import test_gpu_layouts as G
    by_role = {}
    for call, names, off in (("fwd", LU.FWD_TENSORS, 90000), ("bwd", LU.BWD_TENSORS, 92000)):
        seen = {n: set() for n in names}
        for _, seed, case in G.sweep_cases(call):
            for n, L in LU.draw_layouts(np.random.RandomState(off + seed), case, names, seed).items():
                seen[n].add(L.kind)
                by_role.setdefault(LU.ROLE[n], set()).add(L.kind)
        for n in names:
            want = set(LU.kinds_for(LU.ROLE[n], 2)) - {"contig", "batch_gap"}        # (B == 1 cases replace those two)
            assert seen[n] >= want, f"{call} {n}: never drawn: {want - seen[n]}"
    for role, kinds in by_role.items():
        assert kinds >= set(LU.kinds_for(role, 1)), f"{role}: never drawn: {set(LU.kinds_for(role, 1)) - kinds}"


def test_sentinels_are_nan_and_survive_a_round_trip():
    for dt, bits in LU.SENTINEL.items():
        t = torch.full((4,), bits, dtype=LU._RAW[dt]).view(dt)
        assert bool(torch.isnan(t).all()) and bool(LU.is_sentinel(t).all())
        assert not bool(LU.is_sentinel(torch.full((4,), float("nan"), dtype=dt)).any()), "a computed NaN must not look untouched"
