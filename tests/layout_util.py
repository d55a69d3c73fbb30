"""Layout harness: every tensor of a C-ABI call in its own memory layout, inside a sentinel-filled arena.

include/usp_hip.h lets each tensor of a call carry its own pointer and its own stride triple, and every kernel re-derives its
addresses from them.  A test whose tensors are all contiguous gives K and V (dK and dV, q and dout, out and acc, lse and
delta) IDENTICAL strides, so a kernel that addresses V with K's stride passes it.  Here `place` puts a tensor into an arena
under a layout drawn per tensor (`draw_layouts`), the case runners (`check_fwd_case`, `check_bwd_case`, `check_delta_case`,
`check_packed_case`) run a call once with every tensor contiguous and once with the drawn layouts and require

  1. bit-identical outputs between the two runs (the kernels are deterministic and their work split depends on shapes and
     flags only: the required difference is zero),
  2. the contiguous run within golden_util.TOL / long_sum_atol of the fp64 oracle,
  3. every arena element outside the views still the sentinel, and every input view bitwise what was put there,
  4. the header's "not touched" promises, visible through the sentinel (non-final `out` rows, final `acc` rows, the outputs
     of a skipped backward launch, padding between heads).

The module works on torch tensors of any device: tests/test_layouts_cpu.py drives the same runners against the CPU oracle
backend (tests/oracle_backend.py) and against deliberately wrong wrappers of it, which must fail.

Sentinels are NaN bit patterns no arithmetic produces (bf16 0x7FC1, fp16 0x7E01, fp32 0x7FC00001) and are compared as raw
bits: an input read outside a view poisons the result, and a NaN a kernel computed itself is not mistaken for "untouched".
"""
import numpy as np
import torch

from golden_util import TOL, assert_close, long_sum_atol, round_to
from oracle import usp_oracle as O

SENTINEL = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01, torch.float32: 0x7FC00001}
_RAW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}


def raw_bits(t):
    """The elements of `t` (any strides) as a contiguous integer tensor of the same shape."""
    return t.contiguous().view(_RAW[t.dtype])


def is_sentinel(t):
    """Element-wise: does the element still hold the arena's sentinel (raw bits)?"""
    return raw_bits(t) == SENTINEL[t.dtype]


def _up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------------------------------
class Layout:
    """A layout kind + its drawn parameters.  `role` fixes the alignment rules of include/usp_hip.h:
         in16   16-bit input   (pointer and strides multiples of 16 bytes = 8 elements)
         f32    fp32 tensor    (16 bytes = 4 elements)
         out16  16-bit output  (8 bytes = 4 elements: the kernels keep a narrow store path for these)
         lse    (B,H,S) / (H,T) fp32 row statistics (unit seq stride, 4-byte aligned base)."""

    def __init__(self, kind, role, **p):
        self.kind, self.role, self.p = kind, role, p

    def __repr__(self):
        return f"{self.kind}{self.p if self.p else ''}"


ALIGN = {"in16": 8, "f32": 4, "out16": 4}
KINDS4 = ("contig", "seq_major", "head_major", "head_slice", "pack3", "row_pad", "batch_gap", "base_off")
KINDS_B1 = ("b1_zero", "b1_any")                           # B == 1: stride_b is never multiplied by anything but 0
KINDS_OUT16 = ("base8", "stride4")                         # the 8-byte alignment the narrow store paths exist for
KINDS_LSE = ("contig", "hbs", "h_pad", "base4", "s_slice", "batch_gap")


def kinds_for(role, B):
    if role == "lse":
        return KINDS_LSE + (KINDS_B1 if B == 1 else ())
    return KINDS4 + (KINDS_OUT16 if role == "out16" else ()) + (KINDS_B1 if B == 1 else ())


def contiguous(role):
    return Layout("contig", role)


def draw_layout(rs, role, B, kind=None):
    """One layout for a tensor of `role` with batch size B, parameters included.  `kind`: given instead of drawn."""
    kinds = kinds_for(role, B)
    kind = str(kinds[rs.randint(len(kinds))]) if kind is None else kind
    assert kind in kinds, (kind, role, B)
    r = lambda lo, hi: int(rs.randint(lo, hi))
    p = {}
    if role == "lse":
        p = {"h_pad": dict(pad=r(1, 40)), "base4": dict(k=2 * r(0, 4) + 1), "s_slice": dict(extra=r(1, 50), s0=0),
             "batch_gap": dict(gap=r(1, 100)), "b1_any": dict(any=r(1, 10 ** 6))}.get(kind, {})
        if kind == "s_slice":
            p["s0"] = r(0, p["extra"] + 1)
        return Layout(kind, role, **p)
    p = {"head_slice": dict(extra=r(1, 4), h0=0), "pack3": dict(i=r(0, 3)), "row_pad": dict(pad=r(1, 6)),
         "batch_gap": dict(gap=r(1, 50)), "base_off": dict(k=r(1, 20)), "b1_any": dict(any=r(1, 10 ** 5)),
         "base8": dict(k=r(0, 8))}.get(kind, {})
    if kind == "head_slice":
        p["h0"] = r(0, p["extra"] + 1)
    return Layout(kind, role, **p)


def strides4(L, B, S, H, D, ss_mult=1):
    """(stride_b, stride_s, stride_h, offset, extent) in elements of a (B,S,H,D) view under layout L.  `ss_mult`: the
    sequence stride is padded up to a multiple of it (the 64-row kernels need stride_s % 128 == 0 on some inputs)."""
    a, k, p, off = ALIGN[L.role], L.kind, L.p, 0
    if k in ("contig", "batch_gap", "b1_zero", "b1_any", "base_off", "base8"):
        sh = D
        ss = _up(H * sh, ss_mult)
        sb = S * ss
        if k == "batch_gap":
            sb += a * p["gap"]
        elif k == "b1_zero":
            sb = 0
        elif k == "b1_any":
            sb = a * p["any"]
        elif k == "base_off":
            off = a * p["k"]
        elif k == "base8":
            off = 4 * (2 * p["k"] + 1)                      # 8 (mod 16) bytes
    elif k == "seq_major":                                  # (S,B,H,D)
        sh, sb = D, H * D
        ss = _up(B * sb, ss_mult)
    elif k == "head_major":                                 # (B,H,S,D)
        ss = _up(D, ss_mult)
        sh = S * ss
        sb = H * sh
    elif k == "head_slice":                                 # heads h0 : h0 + H of a wider tensor
        sh = D
        ss = _up((H + p["extra"]) * D, ss_mult)
        sb, off = S * ss, p["h0"] * D
    elif k == "pack3":                                      # (B,S,3,H,D)[:, :, i]
        sh = D
        ss = _up(3 * H * D, ss_mult)
        sb, off = S * ss, p["i"] * H * D
    elif k == "row_pad":                                    # stride_h = D + pad
        sh = D + a * p["pad"]
        ss = _up(H * sh, ss_mult)
        sb = S * ss
    elif k == "stride4":                                    # every stride 4 (mod 8) elements: rows only 8-byte aligned
        assert L.role == "out16" and ss_mult == 1
        sh = D + 4
        ss = H * sh + (4 if (H * sh) % 8 == 0 else 0)
        sb = S * ss + (4 if (S * ss) % 8 == 0 else 0)
    else:
        raise ValueError(k)
    assert B == 1 or k not in KINDS_B1
    extent = off + (B - 1) * sb * (B > 1) + (S - 1) * ss + (H - 1) * sh + D
    return sb, ss, sh, off, extent


def strides_lse(L, B, H, S):
    """(stride_b, stride_h, offset, extent) in elements of a (B,H,S) fp32 view with unit seq stride."""
    k, p, off = L.kind, L.p, 0
    sh, sb = S, H * S
    if k == "hbs":                                          # (H,B,S)
        sb, sh = S, B * S
    elif k == "h_pad":                                      # stride_h > S
        sh = S + p["pad"]
        sb = H * sh
    elif k == "base4":                                      # base only 4-byte aligned
        off = p["k"]
    elif k == "s_slice":                                    # a slice along S of a longer sequence
        sh = S + p["extra"]
        sb, off = H * sh, p["s0"]
    elif k == "batch_gap":
        sb += p["gap"]
    elif k == "b1_zero":
        sb = 0
    elif k == "b1_any":
        sb = p["any"]
    elif k != "contig":
        raise ValueError(k)
    extent = off + (B - 1) * sb * (B > 1) + (H - 1) * sh + S
    return sb, sh, off, extent


class Arena:
    """Sentinel-filled device memory holding the views of one call.  Every view gets a slab of its own with guard bands in
    front of and behind it (so no two views can overlap and a tile that overshoots a tensor by its full height at a small
    stride lands in sentinels, not in another tensor).  `untouched()`: every element outside the views is still the
    sentinel; `unchanged(view)`: an input view is bitwise what `place` put there."""
    FRONT, BACK = 16 * 1024, 64 * 1024                      # elements; both multiples of 128: slabs stay 256-byte aligned

    def __init__(self, device):
        self.device = torch.device(device)
        self.slabs = []                                     # (name, raw int buffer, bool mask of the view's elements)
        self._saved = []                                    # (view, its bits at placement)

    def carve(self, name, dtype, shape, strides, offset, extent):
        n = self.FRONT + extent + self.BACK
        raw = torch.full((n,), SENTINEL[dtype], dtype=_RAW[dtype], device=self.device)
        owned = torch.zeros(n, dtype=torch.bool, device=self.device)
        start = self.FRONT + offset
        owned.as_strided(shape, strides, start).fill_(True)
        self.slabs.append((name, raw, owned, SENTINEL[dtype]))
        return raw.view(dtype).as_strided(shape, strides, start)

    def remember(self, view):
        self._saved.append((view, raw_bits(view).clone()))

    def unchanged(self, view=None):
        """The input view (default: every placed input) still holds, bit for bit, what was put there."""
        todo = [(v, b) for v, b in self._saved if view is None or v is view]
        assert todo, "not a placed input of this arena"
        return all(bool(torch.equal(raw_bits(v), b)) for v, b in todo)

    def violations(self):
        """Names of the slabs with an element outside the view that is no longer the sentinel (slab by slab: one boolean
        mask over everything would not index past 2^31 elements)."""
        bad = []
        for name, raw, owned, sentinel in self.slabs:
            hit = (raw != sentinel) & ~owned
            if bool(hit.any()):
                first = int(hit.to(torch.uint8).argmax())
                bad.append(f"{name} (element {first - self.FRONT} from the slab's data start)")
        return bad

    def untouched(self):
        return not self.violations()


def _view_dims(shape, role):
    """(B,S,H,D) of a 4-D or token (T,H,D) tensor; (B,H,S) of an lse or packed (H,T) one."""
    if role == "lse":
        return (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
    return (1,) + tuple(shape) if len(shape) == 3 else tuple(shape)


def blank(shape, dtype, layout, arena, name="?", ss_mult=1):
    """A view of `shape` under `layout` whose every element is the sentinel (an output; an element a kernel never
    writes stays recognisable)."""
    dims = _view_dims(shape, layout.role)
    if layout.role == "lse":
        assert dtype == torch.float32
        B, H, S = dims
        sb, sh, off, extent = strides_lse(layout, B, H, S)
        v = arena.carve(name, dtype, (B, H, S), (sb, sh, 1), off, extent)
    else:
        B, S, H, D = dims
        sb, ss, sh, off, extent = strides4(layout, B, S, H, D, ss_mult)
        v = arena.carve(name, dtype, (B, S, H, D), (sb, ss, sh, 1), off, extent)
    return v[0] if len(shape) == len(dims) - 1 else v


def place(x, layout, arena, name="?", ss_mult=1, track=True):
    """A view under `layout` inside `arena` holding a copy of `x` ((B,S,H,D), (T,H,D), (B,H,S) or (H,T)); with `track`
    the bits are remembered for `arena.unchanged`."""
    v = blank(tuple(x.shape), x.dtype, layout, arena, name, ss_mult)
    v.copy_(x)
    if track:
        arena.remember(v)
    return v


# ------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------
FWD_TENSORS = ("q", "k", "v", "out", "acc", "lse")
BWD_TENSORS = ("dout", "q", "k", "v", "dq", "dk", "dv", "dq16", "dk16", "dv16", "lse", "delta")
ROLE = {"q": "in16", "k": "in16", "v": "in16", "dout": "in16", "o": "in16", "out": "out16", "acc": "f32", "dq": "f32",
        "dk": "f32", "dv": "f32", "dq16": "out16", "dk16": "out16", "dv16": "out16", "lse": "lse", "delta": "lse",
        "blk_out": "in16", "blk_lse": "lse"}


class Case:
    """One call: shapes, flags and (for the backward) the form of each gradient output:
         "f32"     dX  = block                (fp32)
         "f32+"    dX += block                (fp32, accum)
         "h16"     dX16 = round(block)        (16-bit final, fp32 tensor absent)
         "h16+"    dX16 = round(dX + block)   (accum + 16-bit final: dX is read, not written)
    `ring` = (keys of the first call, final_begin, final_end): two forward calls, the second with merge_in.
    `ss128`: names of the tensors whose stride_s must be a multiple of 128 elements (64-row family)."""

    def __init__(self, B, Sq, Sk, Hq, Hkv, D, causal, dt, window=None, softcap=None, k_splits=0, ring=None, family=None,
                 forms=("h16", "h16", "h16"), only=None, splits=(0, 0), dkdv_heads=0, ss128=(), kinds=None):
        self.B, self.Sq, self.Sk, self.Hq, self.Hkv, self.D, self.causal, self.dt = B, Sq, Sk, Hq, Hkv, D, causal, dt
        self.window, self.softcap, self.k_splits, self.ring, self.family = window, softcap, k_splits, ring, family
        self.forms, self.only, self.splits, self.dkdv_heads, self.ss128 = tuple(forms), only, splits, dkdv_heads, tuple(ss128)
        self.kinds = kinds                                  # expected last_launch_kinds() (a set), or None
        self.scale = D ** -0.5

    def __repr__(self):
        keys = ("B", "Sq", "Sk", "Hq", "Hkv", "D", "causal", "dt", "window", "softcap", "k_splits", "ring", "family", "forms",
                "only", "splits", "dkdv_heads")
        return "Case(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in keys) + ")"


def draw_layouts(rs, case, names, index):
    """A layout per tensor name for case number `index` of a sweep.  The KIND is stratified: tensor j walks its role's kinds
    in an order of its own (a fixed permutation per tensor name), one step per case, so that a sweep of a few dozen cases
    shows every tensor every kind while any two tensors of a call keep meeting in different kinds; the parameters are drawn
    from `rs`.  At B == 1 the batch-stride kinds take the place of the two kinds that differ from them only in stride_b.
    (Every kind stays legal when a tensor in case.ss128 has its sequence stride padded to 128 elements: the pad goes
    behind every row.)"""
    out = {}
    for n in names:
        role = ROLE[n]
        base = kinds_for(role, 2)
        perm = np.random.RandomState(sum(map(ord, n))).permutation(len(base))
        kind = base[perm[index % len(base)]]
        if case.B == 1:
            kind = {"contig": "b1_zero", "batch_gap": "b1_any"}.get(kind, kind)
        out[n] = draw_layout(rs, role, case.B, kind)
    return out


def contiguous_layouts(names):
    return {n: contiguous(ROLE[n]) for n in names}


def _tt(x, dt, device):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(getattr(torch, dt)).to(device)


def _host(t):
    return t.detach().contiguous().cpu()


def _f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def make_inputs(case, seed):
    """(q, k, v, dout) as float32 numpy arrays rounded to the case's 16-bit type (softcap cases scale q up so that the cap
    bites, as tests/test_softcap_cpu.py:make_case does)."""
    rs = np.random.RandomState(seed)
    c = case
    q, k, v, do = (round_to(rs.standard_normal(s).astype(np.float32), c.dt)
                   for s in [(c.B, c.Sq, c.Hq, c.D), (c.B, c.Sk, c.Hkv, c.D), (c.B, c.Sk, c.Hkv, c.D), (c.B, c.Sq, c.Hq, c.D)])
    if c.softcap:
        q = round_to(q * 4.0, c.dt)
    return q, k, v, do


def ref_forward(case, q, k, v, causal=None, window="case"):
    """fp64 (out, lse) of one block call: oracle.usp_oracle, or its softcap restatement (tests/test_softcap_cpu.py)."""
    causal = case.causal if causal is None else causal
    window = case.window if window == "case" else window
    if case.softcap:
        from test_softcap_cpu import ref_fwd
        return ref_fwd(q, k, v, case.scale, case.softcap, causal, window)
    return O.attention_ref(q, k, v, causal, case.scale, **({} if window is None else {"window": window}))


# ------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------
def run_fwd(ops, case, seed, device, layouts):
    """The forward call(s) of `case` under `layouts`; returns the outputs as contiguous host tensors.  Checks promises 3
    and 4 of the module docstring for this run."""
    c = case
    q, k, v, _ = make_inputs(c, seed)
    ar = Arena(device)
    m = lambda n: 128 if n in c.ss128 else 1
    tq, tk, tv = (place(_tt(x, c.dt, device), layouts[n], ar, n, m(n)) for x, n in ((q, "q"), (k, "k"), (v, "v")))
    dt16 = getattr(torch, c.dt)
    shape = (c.B, c.Sq, c.Hq, c.D)
    out = blank(shape, dt16, layouts["out"], ar, "out")
    acc = blank(shape, torch.float32, layouts["acc"], ar, "acc")
    lse = blank((c.B, c.Hq, c.Sq), torch.float32, layouts["lse"], ar, "lse")
    kw = dict(window=c.window, softcap=c.softcap, family=c.family)
    what = f"{c} seed {seed} layouts {layouts}"
    kinds = []
    if c.ring is None:
        fb, fe = 0, c.Sq
        ops.fwd(tq, tk, tv, c.scale, c.causal, lse, out=out, acc=None, merge_in=False, final_begin=0, final_end=c.Sq,
                k_splits=c.k_splits, **kw)
        kinds.append(ops.kinds())
    else:
        Sa, fb, fe = c.ring
        ops.fwd(tq, tk[:, :Sa], tv[:, :Sa], c.scale, False, lse, out=None, acc=acc, merge_in=False, final_begin=0,
                final_end=0, k_splits=0, **kw)
        kinds.append(ops.kinds())
        assert not bool(is_sentinel(acc).any()) and not bool(is_sentinel(lse).any()), what + ": first ring call left rows unwritten"
        assert bool(is_sentinel(out).all()), what + ": a call without final rows wrote `out`"
        acc1 = raw_bits(acc).clone()
        ops.fwd(tq, tk[:, Sa:], tv[:, Sa:], c.scale, c.causal, lse, out=out, acc=acc, merge_in=True, final_begin=fb,
                final_end=fe, k_splits=c.k_splits, **kw)
        kinds.append(ops.kinds())
    fin = torch.zeros(c.Sq, dtype=torch.bool, device=out.device)
    fin[fb:fe] = True
    assert not bool(is_sentinel(out[:, fin]).any()), what + ": a final row of `out` was not written"
    assert bool(is_sentinel(out[:, ~fin]).all()), what + ": rows outside [final_begin, final_end) of `out` were written"
    if c.ring is None:
        assert bool(is_sentinel(acc).all()), what + ": `acc` of a call whose rows are all final was written"
    else:
        assert bool(torch.equal(raw_bits(acc)[:, fin], acc1[:, fin])), what + ": accumulator rows of the final range were rewritten"
        assert not bool(is_sentinel(acc[:, ~fin]).any()), what + ": a running row of `acc` was not written"
    assert not bool(is_sentinel(lse).any()), what + ": an lse entry was not written"
    bad = ar.violations()
    assert not bad, what + f": written outside the views: {bad}"
    assert ar.unchanged(), what + ": an input view was modified"
    return dict(out=_host(out), acc=_host(acc), lse=_host(lse), kinds=kinds, fin=fin.cpu())


def assert_same_bits(a, b, what):
    ra, rb = raw_bits(a), raw_bits(b)
    if not torch.equal(ra, rb):
        diff = (ra != rb)
        first = np.unravel_index(int(diff.reshape(-1).to(torch.uint8).argmax()), tuple(diff.shape))
        raise AssertionError(f"{what}: {int(diff.sum())} / {diff.numel()} elements differ in their bits between the contiguous "
                             f"and the strided run; first at {first}: {a[first].item()!r} vs {b[first].item()!r}")


def check_fwd_case(ops, case, seed, device, layouts=None, mutate=None):
    """Contiguous run against the oracle, strided run bit-identical to it.  Returns the launch kinds of the strided run.
    `mutate(results)`: hook of the mutation tests, applied to the strided run's outputs before they are compared."""
    c = case
    layouts = draw_layouts(np.random.RandomState(90000 + seed), c, FWD_TENSORS, seed) if layouts is None else layouts
    what = f"{c} seed {seed}"
    base = run_fwd(ops, c, seed, device, contiguous_layouts(FWD_TENSORS))
    got = run_fwd(ops, c, seed, device, layouts)
    if mutate is not None:
        mutate(got)
    assert base["kinds"] == got["kinds"], f"{what}: the two runs launched different kernels: {base['kinds']} vs {got['kinds']}"
    if c.kinds is not None and base["kinds"][-1] is not None:
        assert set(base["kinds"][-1]) == set(c.kinds), f"{what}: launched {base['kinds'][-1]}, meant {c.kinds}"
    # 2. the contiguous run against the fp64 oracle
    q, k, v, _ = make_inputs(c, seed)
    if c.ring is None:
        ro, rl = ref_forward(c, q, k, v)
    else:
        Sa = c.ring[0]
        o1, l1 = ref_forward(c, q, k[:, :Sa], v[:, :Sa], causal=False)
        o2, l2 = ref_forward(c, q, k[:, Sa:], v[:, Sa:])
        ro, l4 = O.update_out_and_lse(o1, np.swapaxes(l1, 1, 2)[..., None], o2, l2)
        rl = np.swapaxes(l4[..., 0], 1, 2)
    fin_rows = base["fin"].numpy()
    lse = base["lse"].numpy()
    finite = np.isfinite(rl)
    assert (np.isfinite(lse) == finite).all(), what + ": rows without a visible key must give lse = -inf"
    assert_close(lse[finite], rl[finite], 2e-3, 1e-4, what + " lse")
    assert_close(_f64(base["out"][:, fin_rows]), ro[:, fin_rows], *TOL[c.dt]["out"], what + " out")
    if c.ring is not None:
        # fp32 storage, 16-bit arithmetic: P is rounded to the 16-bit type before P V (2^-9 relative in bf16, times |v| up
        # to ~4 when a row sees a handful of keys: 3e-3 observed at Sk = 8), so a running row carries the stated error of
        # 16-bit attention, not that of an fp32 computation
        assert_close(_f64(base["acc"][:, ~fin_rows]), ro[:, ~fin_rows], *TOL[c.dt]["out"], what + " running rows (fp32)")
    # 1. bit-identical between the layouts
    for n in ("out", "acc", "lse"):
        assert_same_bits(base[n], got[n], f"{what} layouts {layouts}: {n}")
    return got["kinds"]


# ------------------------------------------------------------------------------------------------------------------------
# delta + backward
# ------------------------------------------------------------------------------------------------------------------------
def run_delta(ops, case, seed, device, layouts):
    c = case
    _, _, _, do = make_inputs(c, seed)
    o = round_to(np.random.RandomState(seed + 17).standard_normal(do.shape).astype(np.float32), c.dt)
    ar = Arena(device)
    tdo = place(_tt(do, c.dt, device), layouts["dout"], ar, "dout")
    to = place(_tt(o, c.dt, device), layouts["o"], ar, "o")
    delta = blank((c.B, c.Hq, c.Sq), torch.float32, layouts["delta"], ar, "delta")
    ops.delta(tdo, to, delta)
    what = f"delta {c} seed {seed} layouts {layouts}"
    assert not bool(is_sentinel(delta).any()), what + ": an entry was not written"
    bad = ar.violations()
    assert not bad, what + f": written outside the views: {bad}"
    assert ar.unchanged(), what + ": an input view was modified"
    return dict(delta=_host(delta), ref=np.einsum("bshd,bshd->bhs", do.astype(np.float64), o.astype(np.float64)))


DELTA_TENSORS = ("dout", "o", "delta")


def check_delta_case(ops, case, seed, device, layouts=None):
    c = case
    layouts = draw_layouts(np.random.RandomState(91000 + seed), c, DELTA_TENSORS, seed) if layouts is None else layouts
    base = run_delta(ops, c, seed, device, contiguous_layouts(DELTA_TENSORS))
    got = run_delta(ops, c, seed, device, layouts)
    # products of two 16-bit values are exact in fp32; each of the D additions rounds at 2^-24 of a partial sum that stays
    # below ~4 sqrt(D) for N(0,1) inputs: D * 2^-24 * 4 sqrt(D) = 3.5e-4 at D = 128, under 1e-4 sqrt(D) = 1.1e-3
    assert_close(base["delta"].numpy(), base["ref"], 1e-4 * c.D ** 0.5, 1e-5, f"delta {c} seed {seed}")
    assert_same_bits(base["delta"], got["delta"], f"delta {c} seed {seed} layouts {layouts}")


def run_bwd(ops, case, seed, device, layouts):
    """usp_bwd_delta + usp_flash_bwd of `case` under `layouts`.  lse comes from the fp64 oracle and `out` is the oracle's
    output rounded to 16 bits (as tests/test_gpu_fuzz.py:_run_dense does), so the backward does not inherit a forward."""
    c = case
    q, k, v, do = make_inputs(c, seed)
    ro, rl = ref_forward(c, q, k, v)
    o16 = round_to(ro.astype(np.float32), c.dt)
    ar = Arena(device)
    m = lambda n: 128 if n in c.ss128 else 1
    dt16 = getattr(torch, c.dt)
    tdo, tq, tk, tv = (place(_tt(x, c.dt, device), layouts[n], ar, n, m(n)) for x, n in ((do, "dout"), (q, "q"), (k, "k"), (v, "v")))
    lse = place(torch.from_numpy(np.ascontiguousarray(rl, dtype=np.float32)).to(device), layouts["lse"], ar, "lse")
    # delta has its own layout; `out` reuses dout's (the delta kernel's own layout sweep is check_delta_case)
    to = place(_tt(o16, c.dt, device), layouts["dout"], ar, "o")
    delta = blank((c.B, c.Hq, c.Sq), torch.float32, layouts["delta"], ar, "delta")
    ops.delta(tdo, to, delta)
    ar.remember(delta)                                     # from here on an input
    what = f"{c} seed {seed} layouts {layouts}"
    res, args, base = {}, {}, {}
    brs = np.random.RandomState(seed + 29)
    wanted = {None: ("dq", "dk", "dv"), "dq": ("dq",), "dkdv": ("dk", "dv")}[c.only]
    for n, form, like in zip(("dq", "dk", "dv"), c.forms, (q, k, k)):
        n16 = n + "16"
        g32 = g16 = None
        if form.endswith("+"):
            base[n] = brs.standard_normal(like.shape).astype(np.float32)
            g32 = place(torch.from_numpy(base[n]).to(device), layouts[n], ar, n, track=form == "h16+")
        elif form == "f32":
            g32 = blank(like.shape, torch.float32, layouts[n], ar, n)
        if form.startswith("h16"):
            g16 = blank(like.shape, dt16, layouts[n16], ar, n16)
        args[n], args[n16] = g32, g16
        args["accum_" + n] = form.endswith("+")
    ops.bwd(tdo, tq, tk, tv, lse, delta, args["dq"], args["dk"], args["dv"], c.scale, c.causal, accum_dq=args["accum_dq"],
            accum_dk=args["accum_dk"], accum_dv=args["accum_dv"], dq16=args["dq16"], dk16=args["dk16"], dv16=args["dv16"],
            window=c.window, softcap=c.softcap, family=c.family, only=c.only, splits=c.splits, dkdv_heads=c.dkdv_heads)
    kinds = ops.kinds()
    for n, form in zip(("dq", "dk", "dv"), c.forms):
        dst = args[n + "16"] if form.startswith("h16") else args[n]
        if n in wanted:
            assert not bool(is_sentinel(dst).any()), f"{what}: an element of {n} ({form}) was not written"
        elif form.endswith("+") and not form.startswith("h16"):
            assert bool(torch.equal(dst.cpu(), torch.from_numpy(base[n]))), f"{what}: {n} of a skipped launch was modified"
        else:
            assert bool(is_sentinel(dst).all()), f"{what}: {n} of a skipped launch was written"
        res[n] = _host(dst)
    bad = ar.violations()
    assert not bad, what + f": written outside the views: {bad}"
    assert ar.unchanged(), what + ": an input view (or the fp32 addend of a 16-bit final) was modified"
    res.update(delta=_host(delta), kinds=kinds, base=base, wanted=wanted, inputs=(q, k, v, do, o16, rl))
    return res


def check_bwd_case(ops, case, seed, device, layouts=None, mutate=None):
    c = case
    layouts = draw_layouts(np.random.RandomState(92000 + seed), c, BWD_TENSORS, seed) if layouts is None else layouts
    what = f"{c} seed {seed}"
    base = run_bwd(ops, c, seed, device, contiguous_layouts(BWD_TENSORS))
    got = run_bwd(ops, c, seed, device, layouts)
    if mutate is not None:
        mutate(got)
    assert base["kinds"] == got["kinds"], f"{what}: the two runs launched different kernels: {base['kinds']} vs {got['kinds']}"
    if c.kinds is not None and base["kinds"] is not None:
        assert set(base["kinds"]) == set(c.kinds), f"{what}: launched {base['kinds']}, meant {c.kinds}"
    q, k, v, do, o16, rl = base["inputs"]
    if c.softcap:
        from test_softcap_cpu import ref_bwd_from
        rdelta = np.einsum("bshd,bshd->bhs", do.astype(np.float64), o16.astype(np.float64))
        refs = ref_bwd_from(do, q, k, v, rl, rdelta, c.scale, c.softcap, c.causal, c.window)
    else:
        refs = O.block_bwd(do, q, k, v, o16, rl, c.scale, c.causal, **({} if c.window is None else {"window": c.window}))
    G = c.Hq // c.Hkv
    for n, r_ in zip(("dq", "dk", "dv"), refs):
        if n not in base["wanted"]:
            continue
        atol, rtol = TOL[c.dt]["grad"]
        atol = long_sum_atol(atol, c.Sk if n == "dq" else c.Sq * G, r_)
        want = r_ + base["base"][n].astype(np.float64) if n in base["base"] else r_
        assert_close(_f64(base[n]), want, atol, rtol, f"{what} {n}")
    for n in ("delta", "dq", "dk", "dv"):
        assert_same_bits(base[n], got[n], f"{what} layouts {layouts}: {n}")
    return got["kinds"]


# ------------------------------------------------------------------------------------------------------------------------
# packed variable-length batches
# ------------------------------------------------------------------------------------------------------------------------
PACKED_TENSORS = BWD_TENSORS + ("out",)                     # token tensors (T,H,D) and (H,T) row statistics


class PackedCase:
    """Sequences of lens_q[i] query / lens_k[i] key rows inside token tensors, with `gaps` unused rows between (and around)
    them: rows no (first, rows) pair names, which no kernel may touch."""

    def __init__(self, lens_q, lens_k, gaps_q, gaps_k, Hq, Hkv, D, causal, dt, forms=("h16", "h16", "h16"), sched=True,
                 softcap=None):
        self.lens_q, self.lens_k, self.gaps_q, self.gaps_k = list(lens_q), list(lens_k), list(gaps_q), list(gaps_k)
        self.Hq, self.Hkv, self.D, self.causal, self.dt = Hq, Hkv, D, causal, dt
        self.forms, self.sched, self.softcap, self.window = tuple(forms), sched, softcap, None
        self.B, self.scale = 1, D ** -0.5                   # (B: the batch size the layout draw sees)

    def tables(self):
        """((first, rows) per sequence, total rows) for the query and the key side."""
        def one(lens, gaps):
            first, t = [], gaps[0]
            for n, g in zip(lens, gaps[1:]):
                first.append(t)
                t += n + g
            return np.stack([first, lens], 1).astype(np.int32), t
        return one(self.lens_q, self.gaps_q), one(self.lens_k, self.gaps_k)

    def __repr__(self):
        return (f"PackedCase(lens_q={self.lens_q}, lens_k={self.lens_k}, gaps_q={self.gaps_q}, gaps_k={self.gaps_k}, Hq={self.Hq}, "
                f"Hkv={self.Hkv}, D={self.D}, causal={self.causal}, dt={self.dt!r}, forms={self.forms}, sched={self.sched}, "
                f"softcap={self.softcap})")


def draw_packed_case(rs, i, max_len=300, dims=(32, 64, 128)):
    """1..5 sequences of unequal lengths (query and key side different in half of the cases), unused rows around them."""
    n = int(rs.randint(1, 6))
    lq = [int(x) for x in rs.randint(1, max_len, size=n)]
    lk = lq if rs.rand() < 0.5 else [int(x) for x in rs.randint(1, max_len, size=n)]
    gq, gk = ([int(x) for x in rs.randint(0, 20, size=n + 1)] for _ in range(2))
    Hkv = int(rs.choice([1, 2]))
    forms = tuple(str(rs.choice(["f32", "f32+", "h16", "h16+"])) for _ in range(3))
    return PackedCase(lq, lk, gq, gk, Hkv * int(rs.choice([1, 2, 4])), Hkv, int(rs.choice(dims)), bool(rs.rand() < 0.7),
                      str(rs.choice(["bfloat16", "float16"])), forms=forms, sched=bool(i % 2 == 0))


def _row_mask(table, total):
    m = np.zeros(total, dtype=bool)
    for first, rows in table:
        m[first:first + rows] = True
    return m


def packed_reference(pc, seed):
    """Inputs (NaN in the rows outside every sequence) and the fp64 reference, sequence by sequence."""
    (sq, Tq), (sk, Tk) = pc.tables()
    rs = np.random.RandomState(seed)
    q, k, v, do = (round_to(rs.standard_normal(s).astype(np.float32), pc.dt)
                   for s in [(Tq, pc.Hq, pc.D), (Tk, pc.Hkv, pc.D), (Tk, pc.Hkv, pc.D), (Tq, pc.Hq, pc.D)])
    if pc.softcap:
        q = round_to(q * 4.0, pc.dt)
    ro, rl = np.zeros((Tq, pc.Hq, pc.D)), np.full((pc.Hq, Tq), -np.inf)
    grads = [np.zeros((Tq, pc.Hq, pc.D)), np.zeros((Tk, pc.Hkv, pc.D)), np.zeros((Tk, pc.Hkv, pc.D))]
    for (a, n), (c, m) in zip(sq, sk):
        if n > 0:
            if m > 0:
                o_i, l_i = ref_forward(pc, q[None, a:a + n], k[None, c:c + m], v[None, c:c + m])
                ro[a:a + n], rl[:, a:a + n] = o_i[0], l_i[0]
    o16 = round_to(ro.astype(np.float32), pc.dt)
    for (a, n), (c, m) in zip(sq, sk):
        if n > 0 and m > 0:
            sl = (do[None, a:a + n], q[None, a:a + n], k[None, c:c + m], v[None, c:c + m])
            if pc.softcap:
                from test_softcap_cpu import ref_bwd_from
                dl = np.einsum("bshd,bshd->bhs", sl[0].astype(np.float64), o16[None, a:a + n].astype(np.float64))
                g = ref_bwd_from(*sl, rl[None, :, a:a + n], dl, pc.scale, pc.softcap, pc.causal, None)
            else:
                g = O.block_bwd(*sl, o16[None, a:a + n], rl[None, :, a:a + n], pc.scale, pc.causal)
            grads[0][a:a + n], grads[1][c:c + m], grads[2][c:c + m] = g[0][0], g[1][0], g[2][0]
    mq, mk = _row_mask(sq, Tq), _row_mask(sk, Tk)
    for x, m in ((q, mq), (do, mq), (k, mk), (v, mk)):
        x[~m] = np.nan                                      # an input row no sequence names poisons whatever reads it
    return dict(q=q, k=k, v=v, do=do, o16=o16, ro=ro, rl=rl, grads=grads, sq=sq, sk=sk, mq=mq, mk=mk)


def run_packed(ops, pc, seed, device, layouts):
    """Packed forward, delta and packed backward under `layouts`; the outputs' rows inside the sequences as host tensors."""
    r = packed_reference(pc, seed)
    what = f"{pc} seed {seed} layouts {layouts}"
    ar = Arena(device)
    dt16 = getattr(torch, pc.dt)
    tq, tk, tv, tdo = (place(_tt(r[x], pc.dt, device), layouts[n], ar, n) for x, n in (("q", "q"), ("k", "k"), ("v", "v"), ("do", "dout")))
    sq, sk = (torch.from_numpy(r[t]).to(device) for t in ("sq", "sk"))
    mq, mk = (torch.from_numpy(r[t]).to(device) for t in ("mq", "mk"))
    Tq, Tk = len(r["mq"]), len(r["mk"])
    out = blank((Tq, pc.Hq, pc.D), dt16, layouts["out"], ar, "out")
    lse = blank((pc.Hq, Tq), torch.float32, layouts["lse"], ar, "lse")
    ops.fwd_packed(tq, tk, tv, sq, sk, max(pc.lens_q), max(pc.lens_k), pc.scale, pc.causal, lse, out=out, sched=pc.sched,
                   softcap=pc.softcap)
    assert not bool(is_sentinel(out[mq]).any()) and not bool(is_sentinel(lse[:, mq]).any()), what + ": a row of a sequence was not written"
    assert bool(is_sentinel(out[~mq]).all()), what + ": `out` rows outside every sequence were written"
    res = dict(out=_host(out[mq]), lse=_host(lse[:, mq]))
    # backward: lse and `out` from the oracle; delta (H,T) by usp_bwd_delta on the token tensors viewed as B = 1
    o_in = np.where(r["mq"][:, None, None], r["o16"], 0.0)
    to = place(_tt(o_in, pc.dt, device), layouts["dout"], ar, "o")
    lse_in = place(torch.from_numpy(np.where(r["mq"][None], r["rl"], 0.0).astype(np.float32)).to(device), layouts["lse"], ar, "lse_in")
    delta = blank((pc.Hq, Tq), torch.float32, layouts["delta"], ar, "delta")
    ops.delta(tdo[None], to[None], delta[None])
    ar.remember(delta)
    args, base = {}, {}
    brs = np.random.RandomState(seed + 29)
    for n, form, like in zip(("dq", "dk", "dv"), pc.forms, (r["q"], r["k"], r["k"])):
        g32 = g16 = None
        if form.endswith("+"):
            base[n] = brs.standard_normal(like.shape).astype(np.float32)
            g32 = place(torch.from_numpy(base[n]).to(device), layouts[n], ar, n, track=form == "h16+")
        elif form == "f32":
            g32 = blank(like.shape, torch.float32, layouts[n], ar, n)
        if form.startswith("h16"):
            g16 = blank(like.shape, dt16, layouts[n + "16"], ar, n + "16")
        args[n], args[n + "16"] = g32, g16
    ops.bwd_packed(tdo, tq, tk, tv, lse_in, delta, sq, sk, max(pc.lens_q), max(pc.lens_k), args["dq"], args["dk"], args["dv"],
                   pc.scale, pc.causal, accum_dq=pc.forms[0].endswith("+"), accum_dk=pc.forms[1].endswith("+"),
                   accum_dv=pc.forms[2].endswith("+"), dq16=args["dq16"], dk16=args["dk16"], dv16=args["dv16"], sched=pc.sched,
                   softcap=pc.softcap)
    # sequences with no row on the other side are skipped entirely: their gradient rows are not touched either
    live_q = _row_mask([t for t, u in zip(r["sq"], r["sk"]) if u[1] > 0 and t[1] > 0], Tq)
    live_k = _row_mask([u for t, u in zip(r["sq"], r["sk"]) if u[1] > 0 and t[1] > 0], Tk)
    for n, form, live in zip(("dq", "dk", "dv"), pc.forms, (live_q, live_k, live_k)):
        dst = args[n + "16"] if form.startswith("h16") else args[n]
        lv = torch.from_numpy(live).to(device)
        assert not bool(is_sentinel(dst[lv]).any()), f"{what}: a row of {n} ({form}) inside a sequence was not written"
        if form == "f32+":
            assert bool(torch.equal(dst[~lv].cpu(), torch.from_numpy(base[n][~live]))), f"{what}: {n} rows outside every sequence were modified"
        else:
            assert bool(is_sentinel(dst[~lv]).all()), f"{what}: {n} rows outside every sequence were written"
        res[n] = _host(dst[lv])
    bad = ar.violations()
    assert not bad, what + f": written outside the views: {bad}"
    assert ar.unchanged(), what + ": an input view was modified"
    res.update(ref=r, base=base, live=(live_q, live_k), delta=_host(delta[:, mq]))
    return res


def check_packed_case(ops, pc, seed, device, layouts=None, mutate=None):
    layouts = draw_layouts(np.random.RandomState(94000 + seed), pc, PACKED_TENSORS, seed) if layouts is None else layouts
    what = f"{pc} seed {seed}"
    base = run_packed(ops, pc, seed, device, contiguous_layouts(PACKED_TENSORS))
    got = run_packed(ops, pc, seed, device, layouts)
    if mutate is not None:
        mutate(got)
    r = base["ref"]
    rl = r["rl"][:, r["mq"]]
    fin = np.isfinite(rl)
    lse = base["lse"].numpy()
    assert (np.isfinite(lse) == fin).all(), what + ": rows without a visible key must give lse = -inf"
    assert_close(lse[fin], rl[fin], 2e-3, 1e-4, what + " lse")
    assert_close(_f64(base["out"]), r["ro"][r["mq"]], *TOL[pc.dt]["out"], what + " out")
    for n, ref, live in zip(("dq", "dk", "dv"), r["grads"], (base["live"][0], base["live"][1], base["live"][1])):
        want = ref[live] + (base["base"][n][live].astype(np.float64) if n in base["base"] else 0.0)
        assert_close(_f64(base[n]), want, *TOL[pc.dt]["grad"], f"{what} {n}")
    for n in ("out", "lse", "delta", "dq", "dk", "dv"):
        assert_same_bits(base[n], got[n], f"{what} layouts {layouts}: {n}")
