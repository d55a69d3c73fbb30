"""The 256-key-item dK/dV kernel (`flash_bwd_dkdv64u_kernel`, `dkdv_keys=256`): dk and dv, densely, where it can go wrong.

One 64-key wave does S, dP, dV and dK for its keys; an item owns 256 keys.  Every case forces `family="row64"`,
`only="dkdv"`, `dkdv_keys=256`, asserts `_C.last_dkdv_item_keys() == 256` and "dkdv_row64" among the kinds, and compares

- against oracle.usp_oracle.block_bwd with golden_util.assert_close at golden_util.grad_tol, and
- against the 128-key kernel (`dkdv_keys=128`) on the same inputs at equal dkdv_heads / dkdv_splits with torch.equal: the
  arithmetic is that kernel's step for step (same tile, half and k-step order; extra leading masked tiles add +-0).

Shapes (B1 Hq8 / Hkv2 D128, G = 4), the smallest that hold every path:
- Sq = Sk = 320: one full 256-key block and a ragged 64-key one (three of its waves own no key) -- plain, masked and ragged
  tiles, waves whose leading tiles are fully masked; causal and full;
- Sq 192 / Sk 448 causal (causal_off > 0: every row sees the first 256 keys) and Sq 448 / Sk 192 causal (causal_off < 0: rows
  0 .. 255 see no key, lse = -inf);
- dkdv_heads in {1, 2, 4} x dkdv_splits in {0, 2}: `reduce_heads` runs exactly when more than one slab is written.  A cut
  divides the query tiles [t_begin, t_end) of an ITEM into equal runs, and under the causal mask t_begin is that of the item's
  first key: the second 128 keys of a 256-key item are cut at other tiles than the 128-key item that owns them, their fp32
  partial sums group differently, and bit-identity is not a property of the two launches there.  Cut causal launches are
  therefore required to be bit-identical on the first 128 keys of every 256-key block (same t_begin, same runs), cut full
  launches (every item sees every tile) and all uncut launches on every key; the oracle judges every key of every case;
- bf16 and fp16; fp32 outputs accumulated into (accum_dk / accum_dv), 16-bit outputs aligned (whole-row-piece stores) and at
  an 8-byte offset (narrow stores); one case with an independent layout per tensor;
- needle inputs (tests/needle_inputs.py) for one case: a lost, doubled or mispaired 64-row tile or 64-key slice shows;
- a mutation: the reference with two of its 64-key slices swapped must be refused by the same comparator;
- `dkdv_keys=256` with a window is USP_EUNSUPPORTED.
"""
import functools

import numpy as np
import pytest
import torch

import needle_inputs as NI
from golden_util import assert_close, grad_tol, round_to
from oracle import usp_oracle as O

pytestmark = pytest.mark.gpu

B, HQ, HKV, D = 1, 8, 2, 128
G = HQ // HKV
SCALE = D ** -0.5
SHAPES = [(320, 320, True), (320, 320, False), (192, 448, True), (448, 192, True)]
DTS = ["bfloat16", "float16"]


@pytest.fixture(scope="module")
def dev():
    from yunchang_amd import _C
    _C.load()
    return torch.device("cuda:0")


def _finish(q, k, v, do, dt, causal):
    ro, rl = O.attention_ref(q, k, v, causal, SCALE)
    o16 = round_to(ro.astype(np.float32), dt)
    _, rdk, rdv = O.block_bwd(do, q, k, v, o16, rl, SCALE, causal)
    out = (q, k, v, do, o16, rl, rdk, rdv)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(dt, Sq, Sk, causal):
    """(q, k, v, do, o16, lse, reference dk, dv): computed once per case, shared, read-only."""
    rs = np.random.RandomState(11)
    q = round_to(rs.standard_normal((B, Sq, HQ, D)).astype(np.float32), dt)
    k = round_to(rs.standard_normal((B, Sk, HKV, D)).astype(np.float32), dt)
    v = round_to(rs.standard_normal((B, Sk, HKV, D)).astype(np.float32), dt)
    do = round_to(rs.standard_normal(q.shape).astype(np.float32), dt)
    return _finish(q, k, v, do, dt, causal)


@functools.lru_cache(maxsize=None)
def needle_case(dt, S, causal):
    rows = NI.sample_rows(S, 10, 0)
    edges = NI.mask_edges(rows, S, S, causal) + NI.key_block_edges(S, S, causal, per=2)
    nd = NI.make(S, S, HQ, HKV, D, dt, 16, seed=3, edges=edges)
    return _finish(nd.q, nd.k, nd.v, nd.do, dt, causal)


def _dev_inputs(c, dt, layout=False):
    dev = torch.device("cuda:0")
    td = getattr(torch, dt)
    t = lambda x: torch.from_numpy(np.array(x, dtype=np.float32, order="C")).to(td).to(dev)
    q, k, v, do, o16 = (t(x) for x in c[:5])
    if layout:                                # an independent layout per tensor (q / dout keep stride_s % 128 == 0)
        def strided(x, pad_h, pad_s, base):
            b, s, h, d = x.shape
            buf = torch.full((b * (s + pad_s) * (h + pad_h) * d + base,), float("nan"), dtype=x.dtype, device=dev)
            view = buf[base:].view(b, s + pad_s, h + pad_h, d)[:, :s, :h]
            view.copy_(x)
            return view
        q, do = strided(q, 1, 3, 8), strided(do, 2, 0, 16)
        k, v = strided(k, 1, 5, 24), strided(v, 3, 1, 8)
    lse = torch.from_numpy(np.array(c[5], dtype=np.float32, order="C")).to(dev)
    return q, k, v, do, o16, lse


def run(c, dt, causal, keys, heads=0, splits=0, form="h16", layout=False, window=None):
    """(dk, dv) float32 numpy of the forced dK/dV launch; `form`: h16 (aligned 16-bit), h16off (16-bit rows at an 8-byte offset), f32acc."""
    from yunchang_amd import _C
    q, k, v, do, o16, lse = _dev_inputs(c, dt, layout)
    dev = q.device
    Sq, Sk = q.shape[1], k.shape[1]
    delta = torch.empty((B, HQ, Sq), dtype=torch.float32, device=dev)
    _C.bwd_delta(do.contiguous(), o16, delta)
    kw = dict(family="row64", only="dkdv", dkdv_keys=keys, dkdv_heads=heads, splits=(0, splits), window=window)
    shape = (B, Sk, HKV, D)
    if form == "f32acc":
        dk = torch.full(shape, 3.0, dtype=torch.float32, device=dev)
        dv = torch.full(shape, -2.0, dtype=torch.float32, device=dev)
        _C.flash_bwd(do, q, k, v, lse, delta, None, dk, dv, SCALE, causal, accum_dk=True, accum_dv=True, **kw)
        res = (dk - 3.0, dv + 2.0)
    else:
        off = 4 if form == "h16off" else 0
        bufs = [torch.full((B * Sk * HKV * D + off,), float("nan"), dtype=q.dtype, device=dev) for _ in range(2)]
        dk, dv = (b_[off:].view(shape) for b_ in bufs)
        assert (dk.data_ptr() % 16 == 0) == (off == 0)
        _C.flash_bwd(do, q, k, v, lse, delta, None, None, None, SCALE, causal, dk16=dk, dv16=dv, **kw)
        res = (dk, dv)
    kinds = _C.last_launch_kinds()
    assert "dkdv_row64" in kinds and "dkdv_wave8" not in kinds, kinds
    assert _C.last_dkdv_item_keys() == keys, (_C.last_dkdv_item_keys(), keys)
    return tuple(x.float().cpu().numpy() for x in res), kinds


def _check(c, dt, causal, what, **kw):
    (dk, dv), kinds = run(c, dt, causal, 256, **kw)
    assert_close(dk, c[6], *grad_tol(dt, G), what + " dk")
    assert_close(dv, c[7], *grad_tol(dt, G), what + " dv")
    (dk1, dv1), _ = run(c, dt, causal, 128, **kw)
    same = np.ones(dk.shape[1], bool)
    if causal and kw.get("splits", 0) > 1:           # the keys whose item is cut at the same tiles in both launches (docstring)
        same = np.arange(dk.shape[1]) % 256 < 128
    assert np.array_equal(dk[:, same], dk1[:, same]), what + ": dk differs from the 128-key kernel's"
    assert np.array_equal(dv[:, same], dv1[:, same]), what + ": dv differs from the 128-key kernel's"
    return kinds


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"Sq{s[0]}-Sk{s[1]}-{'causal' if s[2] else 'full'}")
@pytest.mark.parametrize("dt", DTS)
def test_dkdv256_shapes(dev, dt, shape):
    Sq, Sk, causal = shape
    c = case(dt, Sq, Sk, causal)
    if Sq > Sk and causal:
        assert not np.isfinite(c[5][0, 0, :Sq - Sk]).any()          # the rows that see no key
    _check(c, dt, causal, f"dkdv256 {shape} {dt}", heads=2)


@pytest.mark.parametrize("splits", [0, 2])
@pytest.mark.parametrize("heads", [1, 2, 4])
def test_dkdv256_gqa_runs_and_cuts(dev, heads, splits):
    c = case("bfloat16", 320, 320, True)
    kinds = _check(c, "bfloat16", True, f"dkdv256 heads={heads} splits={splits}", heads=heads, splits=splits)
    assert ("reduce_heads" in kinds) == (not (heads == G and splits == 0)), kinds


def test_dkdv256_cut_full_launch_is_bit_identical(dev):
    c = case("bfloat16", 320, 320, False)
    kinds = _check(c, "bfloat16", False, "dkdv256 full, heads=2 splits=2", heads=2, splits=2)
    assert "reduce_heads" in kinds, kinds


@pytest.mark.parametrize("form", ["h16", "h16off", "f32acc"])
@pytest.mark.parametrize("dt", DTS)
def test_dkdv256_output_forms(dev, dt, form):
    c = case(dt, 320, 320, True)
    kinds = _check(c, dt, True, f"dkdv256 {form} {dt}", heads=G, form=form)
    assert "reduce_heads" not in kinds, kinds                        # the kernel's own stores, not the reduce's


def test_dkdv256_independent_layouts(dev):
    c = case("bfloat16", 192, 448, True)
    _check(c, "bfloat16", True, "dkdv256 strided", heads=G, layout=True)
    _check(c, "bfloat16", True, "dkdv256 strided, head runs", heads=1, layout=True)


def test_dkdv256_needle_inputs(dev):
    c = needle_case("bfloat16", 576, True)
    (dk, dv), _ = run(c, "bfloat16", True, 256, heads=2)
    v = NI.verdicts({"dk": dk, "dv": dv}, {"dk": c[6], "dv": c[7]}, "bfloat16", 576, 576, G)
    print(f"[dkdv256] needle inputs: worst error / bound dk {v['dk'][1]:.3f} dv {v['dv'][1]:.3f}")
    assert v["dk"][0] and v["dv"][0], v
    (dk1, dv1), _ = run(c, "bfloat16", True, 128, heads=2)
    assert np.array_equal(dk, dk1) and np.array_equal(dv, dv1)


def test_dkdv256_sees_swapped_key_slices(dev):
    """The same comparator refuses the reference with the second and third 64-key slice of the first block swapped."""
    c = case("bfloat16", 320, 320, True)
    (dk, dv), _ = run(c, "bfloat16", True, 256, heads=2)
    for got, want, name in ((dk, c[6], "dk"), (dv, c[7], "dv")):
        mut = np.array(want)
        mut[:, 64:128], mut[:, 128:192] = want[:, 128:192], want[:, 64:128]
        with pytest.raises(AssertionError):
            assert_close(got, mut, *grad_tol("bfloat16", G), name + " against swapped key slices")


def test_dkdv256_declines_a_window(dev):
    c = case("bfloat16", 320, 320, True)
    with pytest.raises(RuntimeError, match=r"code -2\b"):
        run(c, "bfloat16", True, 256, heads=2, window=(100, 0))
