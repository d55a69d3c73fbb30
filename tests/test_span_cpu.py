"""Bidirectional spans (bidirectional=) without a GPU: the host planner (ring/doc_blocks.py) against an enumeration of (row, key)
pairs over whole calls and every (rank, kr) block of ring degrees 2 and 4; the usp_span_* tile-range functions of
csrc/usp_tile_range.h against the same kind of enumeration; the C ABI before any launch; the Python surface's refusals and the
off rule; the sensitivity of the GPU tests' inputs (fp64 mutants with one span end or start moved by one fail the GPU tests'
comparison); the basic ring, the layers and the refusals on gloo grids with the fp64 oracle backend (tests/span_ref.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import needle_inputs
import span_ref
from dist_util import run_distributed
from golden_util import TOL, assert_close, grad_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "long-context-attention_amd", "csrc")


# ---- 1. the planner ---------------------------------------------------------------------------------------------------------------
T = 48
# spans on, one before and one after the shard boundaries of P = 2 (24) and P = 4 (12, 24, 36); one longer than a shard of P = 4
PLANS = [(None, [(11, 13)]), (None, [(12, 14), (23, 24), (24, 30)]), (None, [(10, 12), (13, 25), (35, 37)]),
         (None, [(5, 40)]), (None, [(0, 48)]), (None, [(0, 2), (46, 48)]),
         ([0, 5, 24, 41, 48], [(1, 4), (6, 23), (24, 26), (41, 48)]), ([0, 12, 24, 36, 48], "documents"),
         ([0, 1, 2, 30, 48], [(2, 30), (31, 47)]), ([0, 13, 48], [(11, 13), (13, 37)])]


def _pairs(cu, bidirectional):
    if bidirectional == "documents":
        return list(zip(cu[:-1], cu[1:]))
    return bidirectional


def test_planner_whole_calls_and_every_ring_block():
    """The four arrays are monotone int32, (row_lo, row_hi) and (key_lo, key_hi) describe the same set -- the exact transpose --,
    that set is the global definition's restricted to the block, a block is dropped exactly when it is empty, and ring_visible /
    SpanRingPlan agree with the arrays for every (rank, step) of P in {1, 2, 4}."""
    from yunchang_amd.ring import doc_blocks
    for cu, bidir in PLANS:
        plan = doc_blocks.parse_plan(cu, bidir, 1, T)
        truth = span_ref.global_mask(T, cu, _pairs(cu, bidir))[0].numpy()
        for P in (1, 2, 4):
            S = T // P
            crossing = doc_blocks.spans_cross_shards(plan, S, P)
            for r in range(P):
                got = np.zeros((S, T), dtype=bool)
                ring = doc_blocks.SpanRingPlan(plan, S, P, r)
                for step in range(P):
                    kr = (r - step) % P
                    arr = doc_blocks.span_block_arrays(plan[0], plan.spans[0], r * S, S, kr * S, S)
                    want = truth[r * S:(r + 1) * S, kr * S:(kr + 1) * S]
                    assert (arr is None) == (not want.any()) == (not doc_blocks.ring_visible(plan, S, r, step, P)), (cu, bidir, P, r, step)
                    assert (step in ring.steps) == (arr is not None)
                    assert (ring.key_extent(r, step) is None) == (arr is None)
                    if step > 0:
                        peer = doc_blocks.SpanRingPlan(plan, S, P, kr)
                        assert (step in ring.recv) == (step in peer.send) == (arr is not None), "both ends of a transfer agree"
                    if arr is None:
                        continue
                    assert kr <= r or crossing, "a live block above the diagonal needs a span across a shard boundary"
                    for a in arr:
                        assert a.dtype == np.int32 and (np.diff(a) >= 0).all() and a.min() >= 0 and a.max() <= S
                    m1 = span_ref.block_mask(arr[0], arr[1], S, S)[0].numpy()
                    m2 = span_ref.mask_of_keys(arr[2], arr[3], S, S)[0].numpy()
                    assert np.array_equal(m1, m2) and np.array_equal(m1, want), (cu, bidir, P, r, step)
                    # the ABI's own words for the transposes
                    assert np.array_equal(arr[2], [(arr[1] <= j).sum() for j in range(S)])
                    assert np.array_equal(arr[3], [(arr[0] <= j).sum() for j in range(S)])
                    got[:, kr * S:(kr + 1) * S] = m1
                assert np.array_equal(got, truth[r * S:(r + 1) * S]), (cu, bidir, P, r)
                assert ring.steps[0] == 0, "the diagonal block is always live and opens the rows' state"
    # spans longer than a shard make several blocks above the diagonal live
    plan = doc_blocks.parse_plan(None, [(5, 40)], 1, T)
    assert doc_blocks.SpanRingPlan(plan, 12, 4, 0).steps == [0, 1, 2, 3] and doc_blocks.SpanRingPlan(plan, 12, 4, 3).steps == [0, 1, 2, 3]
    assert doc_blocks.SpanRingPlan(doc_blocks.parse_plan(None, [(11, 13)], 1, T), 12, 4, 0).steps == [0, 3]


def test_planner_batch_lists_and_one_upload():
    from yunchang_amd.ring import doc_blocks
    plan = doc_blocks.parse_plan([[0, 5, T], [0, T]], [[(6, 30)], [(0, 3), (40, 48)]], 2, T)
    assert len(plan) == 2 and plan.spans == (((6, 30),), ((0, 3), (40, 48)))
    call = doc_blocks.ring_call(plan, 24, 2, 0, "cpu")
    kw = call.kw(1)                                   # rank 0 against the keys of rank 1: entry 0 sees some, entry 1 none
    assert set(kw) == {"span"} and len(kw["span"]) == 4 and all(t.dtype == torch.int32 and tuple(t.shape) == (2, 24) for t in kw["span"])
    truth = span_ref.global_mask(T, [[0, 5, T], [0, T]], [[(6, 30)], [(0, 3), (40, 48)]], 2)[:, :24, 24:]
    assert torch.equal(span_ref.block_mask(kw["span"][0], kw["span"][1], 24, 24, 2), truth) and not truth[1].any() and truth[0].any()
    assert torch.equal(span_ref.mask_of_keys(kw["span"][2], kw["span"][3], 24, 24, 2), truth)
    assert not call.causal(0, True) and call.visible(0) and call.visible(1)
    # one buffer behind every launch's arrays
    assert len({t.untyped_storage().data_ptr() for step in (0, 1) for t in call.kw(step)["span"]}) == 1
    # one list of spans shared by B lists of documents, and the reverse
    assert len(doc_blocks.parse_plan([[0, 5, T], [0, T]], [(6, 30)], 2, T)) == 2
    assert len(doc_blocks.parse_plan([0, 5, T], [[(6, 30)], [(7, 9)]], 2, T)) == 2
    # a cu_doclens-only call keeps its two arrays and its causal diagonal block
    call = doc_blocks.ring_call(doc_blocks.parse([0, 5, T], 1, T), 24, 2, 1, "cpu")
    assert set(call.kw(0)) == {"doc"} and call.causal(0, True)


def test_parse_plan_the_off_rule_and_every_value_error():
    from yunchang_amd.ring import doc_blocks
    P = doc_blocks.parse_plan
    docs = doc_blocks.parse([0, 3, 8], 2, 8)
    for off in (None, [], (), [(2, 3)], [(0, 1), (5, 6)], torch.zeros(0, 2, dtype=torch.int64), [[], []], [[(1, 2)], []]):
        assert P(None, off, 2, 8) is None, off
        assert P([0, 8], off, 2, 8) is doc_blocks.SINGLE
        assert P([0, 3, 8], off, 2, 8) == docs and doc_blocks.spans_of(P([0, 3, 8], off, 2, 8)) is None
        assert P(docs, off, 2, 8) is docs
    assert P([0, 1, 2, 3, 4, 5, 6, 7, 8], "documents", 1, 8) == doc_blocks.parse(list(range(9)), 1, 8)     # documents of length 1: off
    plan = P(None, [(2, 5)], 2, 8)
    assert isinstance(plan, doc_blocks.Spans) and plan == ((0, 8),) and plan.spans == (((2, 5),),)
    assert P(plan, None, 2, 8) is plan and doc_blocks.parse(plan, 2, 8) is plan
    assert P(None, "documents", 2, 8).spans == (((0, 8),),) and P([0, 3, 8], "documents", 2, 8).spans == (((0, 3), (3, 8)),)
    assert P(None, torch.tensor([[2, 5], [6, 7]]), 1, 8).spans == (((2, 5),),)
    assert P(None, np.array([[[2, 5]], [[1, 4]]]), 2, 8).spans == (((2, 5),), ((1, 4),))
    assert P(None, [[(2, 5)], [(2, 5)]], 2, 8).spans == (((2, 5),),), "equal lists fold into one"
    bad = ([(5, 7), (2, 4)], [(2, 5), (4, 7)], [(2, 2)], [(3, 2)], [(-1, 2)], [(6, 9)], [(2, 5, 7)], [2, 5], [(2.0, 5.0)],
           torch.tensor([[2, 5]], device="meta"), [[(2, 5)]] * 3, "document", "Documents", torch.tensor([2, 5]), 7)
    for b in bad:
        with pytest.raises(ValueError):
            P(None, b, 2, 8)
    with pytest.raises(ValueError, match="document boundary"):
        P([0, 3, 8], [(2, 5)], 2, 8)
    with pytest.raises(ValueError, match="document boundary"):
        P([[0, 8], [0, 3, 8]], [(2, 5)], 2, 8)
    with pytest.raises(ValueError):
        P([0, 3, 7], [(1, 2)], 2, 8)                  # the document list's own errors come first


# ---- 2. the tile ranges, compiled as tests/test_tile_range_cpu.py compiles the header -----------------------------------------------
SHIM = r"""
#define USP_RANGE_FN
#include "usp_tile_range.h"
/* query side: item of BM rows, waves of WAVE rows, 64-key tiles, as the forward and the dQ kernel use the functions.  Per item:
   first tile, end tile; per (wave, tile of [0, ceil(Sk / 64))): unmasked-by-the-right-bound count of the wave (once), live, masked. */
int sweep_query(const int* row_lo, const int* row_hi, int Sq, int Sk, int BM, int WAVE, int* head, int* tiles) {
  const int T = 64, nt_all = (Sk + T - 1) / T;
  int n = 0;
  for (int q0 = 0; q0 < Sq; q0 += BM) {
    const int te = usp_span_key_tiles_end(usp_span_row_hi(row_hi, q0 + BM - 1, Sq, Sk), nt_all, T);
    *head++ = usp_doc_first_key_tile(usp_doc_row_lo(row_lo, q0, Sq, Sk), te, T);
    *head++ = te;
    for (int qw = q0; qw < q0 + BM && qw < Sq; qw += WAVE) {
      const int lo0 = usp_doc_row_lo(row_lo, qw, Sq, Sk), hi0 = usp_span_row_hi(row_hi, qw, Sq, Sk);
      const int hi1 = usp_span_row_hi(row_hi, qw + WAVE - 1, Sq, Sk);
      *tiles++ = usp_span_unmasked_key_tiles(hi0, T);
      for (int t = 0; t < nt_all; ++t) {
        *tiles++ = usp_span_key_tile_live(t * T, T, hi1, lo0);
        *tiles++ = usp_span_key_tile_masked(t * T, T, hi0);
        ++n;
      }
    }
  }
  return n;
}
/* key side: block of OWN keys, waves of WAVE keys, 64-row tiles */
int sweep_key(const int* key_lo, int Sq, int Sk, int OWN, int WAVE, int* head, int* tiles) {
  const int T = 64, nt = (Sq + T - 1) / T;
  int n = 0;
  for (int own0 = 0; own0 < Sk; own0 += OWN) {
    *head++ = usp_span_first_row_tile(usp_span_key_lo(key_lo, own0, Sq, Sk), nt, T);
    for (int ow = own0; ow < own0 + OWN && ow < Sk; ow += WAVE) {
      const int l0 = usp_span_key_lo(key_lo, ow, Sq, Sk), l1 = usp_span_key_lo(key_lo, ow + WAVE - 1, Sq, Sk);
      for (int t = 0; t < nt; ++t) {
        *tiles++ = usp_span_row_tile_live(t * T, T, l0);
        *tiles++ = usp_span_row_tile_masked(t * T, l1);
        ++n;
      }
    }
  }
  return n;
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("spanrange")
    src, lib = d / "shim.c", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.check_call(["gcc", "-O2", "-fno-semantic-interposition", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(lib)])
    return ctypes.CDLL(str(lib))


def _monotone_pairs():
    """(Sq, Sk, row_lo, row_hi): planner output for span lists around multiples of 64, blocks off and above the diagonal, and
    random monotone staircases (what the ABI admits beyond spans), rows that see nothing included."""
    from yunchang_amd.ring import doc_blocks
    rs = np.random.RandomState(1)
    cases = []
    for S, cu, spans in ((320, None, [(62, 64), (64, 67), (127, 129), (190, 193), (250, 262), (300, 320)]),
                         (257, [0, 64, 257], [(1, 63), (65, 256)]), (63, None, [(0, 63)]), (449, [0, 100, 449], [(120, 400)])):
        plan = doc_blocks.parse_plan(cu, spans, 1, S)
        a = doc_blocks.span_block_arrays(plan[0], plan.spans[0], 0, S, 0, S)
        cases.append((S, S, a[0], a[1]))
    plan = doc_blocks.parse_plan(None, [(100, 300), (400, 500)], 1, 768)
    for row0, key0 in ((0, 256), (512, 0), (256, 256)):
        a = doc_blocks.span_block_arrays(plan[0], plan.spans[0], row0, 256, key0, 512)
        cases.append((256, 512, a[0], a[1]))
    for Sq, Sk in ((320, 320), (256, 512), (130, 449), (449, 300)):
        for _ in range(3):
            lo = np.sort(rs.randint(0, Sk + 1, size=Sq))
            hi = np.sort(rs.randint(0, Sk + 1, size=Sq))
            cases.append((Sq, Sk, lo.astype(np.int32), hi.astype(np.int32)))
        cases.append((Sq, Sk, np.zeros(Sq, np.int32), np.full(Sq, Sk, np.int32)))
        cases.append((Sq, Sk, np.full(Sq, Sk, np.int32), np.zeros(Sq, np.int32)))
    return cases


def test_tile_ranges_against_an_enumeration(shim):
    """Every answer of the usp_span_* functions against the (row, key) pairs of row_lo[i] <= j < row_hi[i]: no visible pair falls
    outside the streamed range, no tile counted "unmasked" holds a hidden pair, and the EXACT statements of the header are exact
    -- for the geometries of the kernels: 256 / 128-row items with 32-row waves, the 128-key block with 32-key waves."""
    T = 64
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    for Sq, Sk, lo, hi in _monotone_pairs():
        lo, hi = np.ascontiguousarray(lo, np.int32), np.ascontiguousarray(hi, np.int32)
        j = np.arange(Sk)[None, :]
        left, right = j >= lo[:, None], j < hi[:, None]
        vis = left & right
        key_lo = np.searchsorted(hi, np.arange(Sk), side="right").astype(np.int32)
        assert np.array_equal(right, np.arange(Sq)[:, None] >= key_lo[None, :]), "row_hi and key_lo describe the same set"
        nt_all = -(-Sk // T)
        for BM in (256, 128):
            n_items = -(-Sq // BM)
            head = (ctypes.c_int * (2 * n_items))()
            tiles = (ctypes.c_int * (n_items * (BM // 32) * (2 * nt_all + 1)))()
            shim.sweep_query(ip(lo), ip(hi), Sq, Sk, BM, 32, head, tiles)
            it = iter(tiles)
            for qi, q0 in enumerate(range(0, Sq, BM)):
                rows = slice(q0, min(q0 + BM, Sq))
                t0, te = head[2 * qi], head[2 * qi + 1]
                assert 0 <= t0 <= te <= nt_all
                assert not vis[rows, te * T:].any() and not vis[rows, :t0 * T].any(), "no visible pair outside the streamed range"
                assert te == 0 or right[rows.stop - 1, (te - 1) * T:].any() or hi[rows.stop - 1] > Sk, "the end tile is exact for the last valid row"
                assert te == min(nt_all, -(-int(hi[rows.stop - 1]) // T))
                for qw in range(q0, rows.stop, 32):
                    wr = slice(qw, min(qw + 32, Sq))
                    nf = next(it)
                    assert right[wr, :nf * T].all(), "no tile counted unmasked holds a pair the right bound hides"
                    # (a ragged last tile is never counted: it is masked for its keys past Sk whatever the bound says)
                    assert (nf + 1) * T > Sk or not right[qw, nf * T:(nf + 1) * T].all(), "... and the count is exact for the wave's first row"
                    for t in range(nt_all):
                        live, masked = next(it), next(it)
                        ks = slice(t * T, min(t * T + T, Sk))
                        assert live or not vis[wr, ks].any(), "a tile with a visible pair is live"
                        assert live == bool(t * T < hi[wr.stop - 1] and t * T + T > lo[qw]), "live: each bound alone leaves a pair"
                        hidden = not right[wr, ks].all()
                        assert masked or not hidden, "a tile with a pair the right bound hides is masked (never the reverse error)"
                        assert masked == hidden or ks.stop < t * T + T, "exact for a tile of valid keys"
        n_blk = -(-Sk // 128)
        nt = -(-Sq // T)
        head = (ctypes.c_int * n_blk)()
        tiles = (ctypes.c_int * (2 * n_blk * 4 * nt))()
        shim.sweep_key(ip(key_lo), Sq, Sk, 128, 32, head, tiles)
        it = iter(tiles)
        for bi, own0 in enumerate(range(0, Sk, 128)):
            ks = slice(own0, min(own0 + 128, Sk))
            tb = head[bi]
            assert 0 <= tb <= nt and not right[:tb * T, ks].any(), "no row tile below t_begin sees a key of the block"
            assert tb == nt or right[tb * T:(tb + 1) * T, own0].any() or key_lo[own0] >= Sq, "exact for the block's first key"
            for ow in range(own0, ks.stop, 32):
                kw = slice(ow, min(ow + 32, Sk))
                for t in range(nt):
                    live, masked = next(it), next(it)
                    rows = slice(t * T, min(t * T + T, Sq))
                    assert live or not right[rows, kw].any(), "a tile with a visible pair is live"
                    assert live == bool(t * T + T > key_lo[ow]), "live (this bound alone; rows past Sq count)"
                    assert masked == (not right[rows, kw].all()), "masked: exact for this bound alone"


# ---- 3. the C ABI at the host ------------------------------------------------------------------------------------------------------
def _lib():
    from yunchang_amd import _C
    if not os.path.exists(_C.lib_path()):
        pytest.fail("libusp_hip.so is not built: run __graft_entry__.build() first")
    return _C, _C.load()


def _args(_C, cls, addr):
    a = cls()
    a.dtype, a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D = 0, 1, 16, 16, 2, 2, 128
    a.softmax_scale = 0.125
    a.lse = addr
    if cls is _C.UspBwdArgs:
        a.delta = addr
        a.dout.ptr = addr
    a.q.ptr = a.k.ptr = a.v.ptr = addr
    outs = (a.dq, a.dk, a.dv) if cls is _C.UspBwdArgs else (a.out,)
    if cls is _C.UspFwdArgs:
        a.final_end = a.Sq
    for t in outs:
        t.ptr = addr
    for t in (a.q, a.k, a.v) + outs + ((a.dout,) if cls is _C.UspBwdArgs else ()):
        t.stride_b, t.stride_s, t.stride_h = 16 * 2 * 128, 2 * 128, 128
    return a


def test_abi_feature_bit_entry_points_and_unchanged_structs():
    _C, L = _lib()
    txt = open(os.path.join(ROOT, "include", "usp_hip.h")).read()
    assert _C.USP_ATTN_SPAN == 4096 == int(re.search(r"#define USP_ATTN_SPAN (\d+)", txt).group(1))
    assert L.usp_attn_features() & _C.USP_ATTN_SPAN
    assert L.usp_abi_version() == 7 == _C.ABI_VERSION
    assert (ctypes.sizeof(_C.UspFwdArgs), ctypes.sizeof(_C.UspBwdArgs)) == (296, 504)
    for name in ("usp_flash_fwd_span", "usp_flash_bwd_span"):
        assert name in _C.SPAN_EXPORTS and name in _C.EXPORTS and hasattr(L, name)
        assert _C._span_entry(name).restype is ctypes.c_int
    assert re.search(r"int usp_flash_fwd_span\(const usp_fwd_args\* args, const int32_t\* row_lo, int64_t row_lo_stride_b, "
                     r"const int32_t\* row_hi,\s+int64_t row_hi_stride_b, void\* stream\);", txt)
    assert re.search(r"int usp_flash_bwd_span\(const usp_bwd_args\* args, const int32_t\* row_lo, int64_t row_lo_stride_b, "
                     r"const int32_t\* row_hi,\s+int64_t row_hi_stride_b, const int32_t\* key_lo, int64_t key_lo_stride_b, "
                     r"const int32_t\* key_hi,\s+int64_t key_hi_stride_b, void\* stream\);", txt)
    assert len(re.findall(r"typedef struct", txt)) == 3


def test_abi_declines_without_launch():
    """Host memory stands in for the device pointers (the arrays included): every call below returns before anything is launched.
    The order: the argument checks every call gets; (backward) a launch that runs lacks one of its two arrays; a negative stride;
    then the declines, causal among them."""
    _C, L = _lib()
    buf = ctypes.create_string_buffer(1 << 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    seq = (ctypes.c_int32 * 2)(0, 16)
    arr = (ctypes.c_int32 * 16)()
    ap = ctypes.cast(arr, ctypes.c_void_p)
    fwd, bwd = _C._span_entry("usp_flash_fwd_span"), _C._span_entry("usp_flash_bwd_span")
    fdoc, bdoc = _C._doc_entry("usp_flash_fwd_doc"), _C._doc_entry("usp_flash_bwd_doc")
    calls = ((_C.UspFwdArgs, lambda a, sb=0: fwd(ctypes.byref(a), ap, 0, ap, sb, None), lambda a, sb=0: fwd(ctypes.byref(a), None, -3, ap, sb, None),
              lambda a: L.usp_flash_fwd(ctypes.byref(a), None), lambda a: fwd(ctypes.byref(a), None, -5, None, -5, None)),
             (_C.UspBwdArgs, lambda a, sb=0: bwd(ctypes.byref(a), ap, 0, ap, 0, ap, sb, ap, 0, None),
              lambda a, sb=0: bwd(ctypes.byref(a), ap, 0, ap, sb, ap, 0, ap, 0, None),
              lambda a: L.usp_flash_bwd(ctypes.byref(a), None), lambda a: bwd(ctypes.byref(a), None, -5, None, -5, None, -5, None, -5, None)))
    for cls, call, call2, plain, null in calls:
        for c in (call, call2):
            for causal, flags, extra, want in ((1, 0, {}, -2), (0, _C.USP_ATTN_SOFTCAP, dict(softcap=30.0), -2),
                                               (0, _C.USP_ATTN_WINDOW, dict(window_left=4, window_right=0), -2),
                                               (0, _C.USP_ATTN_SHIFT, dict(mask_shift=0), -2), (0, _C.USP_FORCE_ROW64, {}, -2)):
                a = _args(_C, cls, addr)
                a.causal, a.flags = causal, flags
                for kk, vv in extra.items():
                    setattr(a, kk, vv)
                assert c(a) == want, (cls.__name__, causal, flags)
                assert c(a, -1) == -1, "a negative stride comes before the declines"
                assert L.usp_last_launch_kinds() == 0
            a = _args(_C, cls, addr)                       # a packed batch
            a.seq_q = a.seq_k = ctypes.addressof(seq)
            if cls is _C.UspBwdArgs:
                a.total_k = 16
            assert c(a) == -2
            a = _args(_C, cls, addr)                       # the existing checks still come first
            a.flags, a.softmax_scale = _C.USP_FORCE_ROW64, 0.0
            assert c(a) == -1
        # everything NULL is the plain entry, whatever the strides: the same answer for a call both refuse
        for mut in (dict(softmax_scale=0.0), dict(D=48), dict(Hq=3)):
            a = _args(_C, cls, addr)
            for kk, vv in mut.items():
                setattr(a, kk, vv)
            assert null(a) == plain(a) != 0, mut
        assert L.usp_last_launch_kinds() == 0
    # row_hi == NULL (backward: and key_lo == NULL) is the document entry on the remaining arrays: a causal call is not declined
    # for being causal, and what the document entry declines is declined alike
    for flags, want in ((_C.USP_FORCE_ROW64, -2), (_C.USP_FORCE_ROW64 | _C.USP_FORCE_WAVE32, -1)):
        a = _args(_C, _C.UspFwdArgs, addr)
        a.causal, a.flags = 1, flags
        assert fwd(ctypes.byref(a), ap, 0, None, -9, None) == fdoc(ctypes.byref(a), ap, 0, None) == want
        b = _args(_C, _C.UspBwdArgs, addr)
        b.causal, b.flags = 1, flags
        assert bwd(ctypes.byref(b), ap, 0, None, -9, None, -9, ap, 0, None) == bdoc(ctypes.byref(b), ap, 0, ap, 0, None) == want
    # backward: a launch that is not skipped and lacks one of its two arrays is EINVAL; USP_BWD_SKIP_* lifts it for the skipped launch
    # (a forced 64-row call is then declined as ever: nothing is launched here either)
    b = _args(_C, _C.UspBwdArgs, addr)
    N = None
    for rl, rh, kl, kh in ((ap, ap, N, ap), (ap, ap, ap, N), (N, ap, ap, ap), (ap, ap, N, N), (N, N, ap, ap), (N, ap, N, N), (N, N, ap, N)):
        assert bwd(ctypes.byref(b), rl, 0, rh, 0, kl, 0, kh, 0, None) == -1, (rl, rh, kl, kh)
    b.flags = _C.USP_FORCE_ROW64 | _C.USP_BWD_SKIP_DKDV
    assert bwd(ctypes.byref(b), ap, 0, ap, 0, N, 0, N, 0, None) == -2 and bwd(ctypes.byref(b), N, 0, ap, 0, ap, 0, ap, 0, None) == -1
    b.flags = _C.USP_FORCE_ROW64 | _C.USP_BWD_SKIP_DQ
    assert bwd(ctypes.byref(b), N, 0, N, 0, ap, 0, ap, 0, None) == -2 and bwd(ctypes.byref(b), ap, 0, ap, 0, ap, 0, N, 0, None) == -1
    assert L.usp_last_launch_kinds() == 0


# ---- 4. the Python surface ---------------------------------------------------------------------------------------------------------
def test_python_refusals_and_the_off_rule(monkeypatch):
    from yunchang_amd import _C
    from yunchang_amd.kernels import attention as KA
    from yunchang_amd.kernels.features import Features, SPAN_ON
    from yunchang_amd.ring.ring_flash_attn_varlen import ring_flash_attn_varlen_func
    q = torch.zeros(2, 16, 4, 64, dtype=torch.bfloat16)
    cu, sp = [0, 5, 16], [(6, 9)]
    for bad in ([(9, 6)], [(6, 9), (8, 10)], [(10, 12), (6, 9)], [(4, 6)], [(6, 17)], [[(6, 9)]] * 3, "docs",
                torch.tensor([[6, 9]], device="meta")):
        for call in (lambda: KA.hip_attn_func(q, q, q, causal=True, cu_doclens=cu, bidirectional=bad),
                     lambda: KA.hip_attn_forward(q, q, q, causal=True, cu_doclens=cu, bidirectional=bad)):
            with pytest.raises(ValueError):
                call()
    for kw in (dict(cu_doclens=cu), {}):
        with pytest.raises(NotImplementedError, match="bidirectional needs causal=True"):
            KA.hip_attn_func(q, q, q, causal=False, bidirectional=sp, **kw)
        with pytest.raises(NotImplementedError, match="bidirectional needs causal=True"):
            KA.hip_attn_func(q, q[:, :8], q[:, :8], causal=True, bidirectional=[(2, 4)])
        for extra, what in ((dict(window_size=(4, 0)), "window_size"), (dict(softcap=30.0), "softcap"), (dict(alibi_slopes=torch.rand(4)), "alibi_slopes"),
                            (dict(dropout_p=0.1), "dropout_p"), (dict(sinks=torch.zeros(4)), "sinks")):
            for fn in (KA.hip_attn_func, KA.hip_attn_forward):
                with pytest.raises(NotImplementedError, match=f"bidirectional together with {what} is not supported by the HIP attention kernels"):
                    fn(q, q, q, causal=True, bidirectional=sp, **kw, **extra)
    # off: exactly the call without the keyword -- the same record, the verdicts of cu_doclens alone
    for off in (None, [], [(6, 7)]):
        assert Features.of(q, q, True, cu_doclens=cu, bidirectional=off) == Features.of(q, q, True, cu_doclens=cu)
        assert Features.of(q, q, False, bidirectional=off) == Features.of(q, q, False)
        with pytest.raises(NotImplementedError, match="cu_doclens together with softcap"):
            Features.of(q, q, True, softcap=30.0, cu_doclens=cu, bidirectional=off)
    assert Features._fields == ("window", "softcap", "alibi", "dropout", "sinks", "doc"), "the spans ride inside `doc`: no seventh field"
    with pytest.raises(NotImplementedError, match="bidirectional together with softcap"):
        Features(softcap=30.0, doc=SPAN_ON).check()
    # the wrapper: dense calls hand the per-launch arrays on as span= and refuse a launch without them; packed ones refuse
    seen = {}

    class Rec:
        def fwd(self, *a, **kw):
            seen["fwd"] = kw

        def bwd(self, *a, **kw):
            seen["bwd"] = kw
    prev = KA.set_block_backend(Rec())
    try:
        be = KA.get_block_backend(doc=SPAN_ON)
        be.fwd(1, span=("a", "b", "c", "d"))
        be.bwd(2, span=("a", "b", "c", "d"), only="dq")
        assert seen["fwd"] == {"span": ("a", "b", "c", "d")} and seen["bwd"] == {"span": ("a", "b", "c", "d"), "only": "dq"}
        with pytest.raises(RuntimeError):
            be.fwd(1)
        for packed in (be.fwd_packed, be.bwd_packed):
            with pytest.raises(NotImplementedError, match="bidirectional is not supported on packed"):
                packed()
    finally:
        KA.set_block_backend(prev)
    cs = torch.tensor([0, 16], dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="bidirectional.*ring_flash_attn_func on dense batches"):
        ring_flash_attn_varlen_func(q[0], q[0], q[0], cs, 16, causal=True, bidirectional=sp)
    # the array checks of the binding
    cpu = torch.device("cpu")
    r1, r2 = torch.zeros(16, dtype=torch.int32), torch.zeros(2, 16, dtype=torch.int32)
    assert _C.span_value(None, 2, 16, 16, cpu) is None and _C.span_value((None,) * 4, 2, 16, 16, cpu) is None
    assert _C.span_value((r1, r2, None, r1), 2, 16, 16, cpu) == ((r1, 0), (r2, 16), (None, 0), (r1, 0))
    for bad in ((r1.long(), r1, r1, r1), (r1[:8], r1, r1, r1), (r1, r2.T, r1, r1), (r1, [0] * 16, r1, r1), (r1, r1, r1.to("meta"), r1), (r1, r1)):
        with pytest.raises(ValueError):
            _C.span_value(bad, 2, 16, 16, cpu)
    # a library without the feature bit
    L = _C.load()

    class Old:
        def __getattr__(self, name):
            return getattr(L, name)

        def usp_attn_features(self):
            return L.usp_attn_features() & ~_C.USP_ATTN_SPAN
    monkeypatch.setattr(_C, "_lib", Old())
    with pytest.raises(NotImplementedError, match=r"bidirectional \(USP_ATTN_SPAN\): rebuild it"):
        _C._span_entry("usp_flash_fwd_span")


# ---- 5. sensitivity: the GPU tests' inputs see one span end or start moved by one -----------------------------------------------------
def _mutants(spans, cu, S):
    """Every span of two or more positions with its start or its end moved by one, each way, where the list stays a valid one
    (sorted, disjoint, inside one document, still of length >= 1)."""
    bounds = cu or [0, S]
    doc_of = lambda p: max(i for i, b in enumerate(bounds[:-1]) if b <= p)
    out = []
    for n, (s, e) in enumerate(spans):
        if e - s < 2:
            continue
        prev_e = spans[n - 1][1] if n else 0
        next_s = spans[n + 1][0] if n + 1 < len(spans) else S
        for ns, ne in ((s - 1, e), (s + 1, e), (s, e - 1), (s, e + 1)):
            if ns < prev_e or ne > next_s or ns < 0 or ne > S or ne - ns < 1 or doc_of(ns) != doc_of(ne - 1):
                continue
            out.append(((s, e), (ns, ne), spans[:n] + [(ns, ne)] + spans[n + 1:]))
    return out


@pytest.mark.parametrize("S,D,dt,Hq,Hkv,kind", [(320, 64, "bfloat16", 4, 1, "alone"), (320, 32, "bfloat16", 4, 4, "in-docs"),
                                                (1280, 128, "bfloat16", 4, 1, "alone"), (320, 128, "float16", 4, 1, "documents"),
                                                (320, 64, "float16", 4, 4, "alone")], ids=lambda v: str(v))
def test_span_mutants_fail(S, D, dt, Hq, Hkv, kind):
    """On the inputs of tests/test_gpu_span.py (needle_inputs.make with span_ref.needle_edges), an fp64 reference with ONE span
    end or start moved by ONE key / row, each way, fails the GPU tests' comparison (golden_util.TOL for out, grad_tol for every
    gradient) in out, dq, dk and dv.  Mutants that would not be a valid list (they touch a neighbouring span or cross a document
    boundary) are not formed; every span of two or more positions keeps at least one mutant of its start and one of its end."""
    import test_gpu_span as G
    cu, _, pairs = G._kind(kind, S)
    pairs = list(pairs)
    nd = needle_inputs.make(S, S, Hq, Hkv, D, dt, C=8, seed=S + D, edges=span_ref.needle_edges(pairs, S, cu))
    q, k, v, do = (torch.from_numpy(x.astype(np.float32)).to(getattr(torch, dt)) for x in (nd.q, nd.k, nd.v, nd.do))
    scale = D ** -0.5
    true = span_ref.ref_bwd(do, q, k, v, scale, span_ref.global_mask(S, cu, pairs), out_dtype=q.dtype)
    muts = _mutants(pairs, cu, S)
    for sp in pairs:
        if sp[1] - sp[0] >= 2:
            mine = [m for m in muts if m[0] == sp]
            assert any(m[1][0] != sp[0] for m in mine) or sp[0] == 0 or cu is not None, f"span {sp}: no mutant of its start"
            assert any(m[1][1] != sp[1] for m in mine), f"span {sp}: no mutant of its end"
    assert len(muts) >= 2 * sum(1 for s, e in pairs if e - s >= 2)
    for sp, moved, mut in muts:
        wrong = span_ref.ref_bwd(do, q, k, v, scale, span_ref.global_mask(S, cu, mut), out_dtype=q.dtype)
        for name, a, b, tol in (("out", wrong[0], true[0], TOL[dt]["out"]), ("dq", wrong[2], true[2], grad_tol(dt, Hq // Hkv)),
                                ("dk", wrong[3], true[3], grad_tol(dt, Hq // Hkv)), ("dv", wrong[4], true[4], grad_tol(dt, Hq // Hkv))):
            ok, ratio = needle_inputs.bound_ratio(a.numpy(), b.numpy(), *tol)
            assert not ok and ratio > 1.0, f"S{S} D{D} {kind}: span {sp} -> {moved} passes in {name} (worst err / bound {ratio:.2f})"


# ---- 6. gloo grids with the oracle backend -------------------------------------------------------------------------------------------
B, HQ, HKV, DH, TG = 2, 4, 2, 32, 96
SCALE = DH ** -0.5
CU_GRID = [[0, 1, 30, 96], [0, 47, 96]]
# entry 0: a span across the shard boundaries 48 (P = 2) and 72 (P = 4) that is longer than a shard of P = 4; entry 1: a span
# across 24 and one ending at the sequence end
SP_GRID = [[(2, 20), (40, 80)], [(20, 30), (60, 96)]]


def _inputs():
    g = torch.Generator().manual_seed(13)
    return [torch.randn(B, TG, h, DH, generator=g).to(torch.bfloat16) for h in (HQ, HKV, HKV, HQ)]


def _truth():
    q, k, v, do = _inputs()
    r = span_ref.ref_bwd(do, q, k, v, SCALE, span_ref.global_mask(TG, CU_GRID, SP_GRID, B), out_dtype=torch.bfloat16)
    return (r[0],) + r[2:]


def _grads(out, leaves, do):
    out.backward(do)
    return [t.detach().float().numpy() for t in (out,) + tuple(x.grad for x in leaves)]


def _worker(rank, ws, ud, rd):
    import torch.distributed as dist
    import yunchang_amd as Y
    from yunchang_amd.kernels import set_block_backend
    from yunchang_amd.ring import doc_blocks, ring_flash_attn_func
    from yunchang_amd.ring.ring_flash_attn_varlen import ring_flash_attn_varlen_func
    import yunchang_amd.hybrid.attn_layer as AL
    be = span_ref.SpanOracleBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    piped = []

    class Counted:
        apply = staticmethod(lambda *a, _f=AL._AsyncUSPFunc.apply: (piped.append(a[8]), _f(*a))[1])
    AL._AsyncUSPFunc = Counted
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    loc = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in _inputs()]
    res = {"cases": {}, "refused": [], "logs": {}, "piped": {}, "spans": {}}

    def leaves():
        return [t.detach().clone().requires_grad_(True) for t in loc[:3]]
    layer = Y.LongContextAttention(ring_impl_type="basic")
    for name, kw in (("layer", dict(cu_doclens=CU_GRID, bidirectional=SP_GRID)), ("none", {}), ("off_empty", dict(bidirectional=[])),
                     ("off_len1", dict(bidirectional=[(3, 4), (50, 51)])), ("doc", dict(cu_doclens=CU_GRID)),
                     ("doc_off", dict(cu_doclens=CU_GRID, bidirectional=[[(3, 4)], []]))):
        del be.doc_log[:], be.span_log[:], piped[:]
        lv = leaves()
        res["cases"][name] = _grads(layer(*lv, causal=True, **kw), lv, loc[3])
        res["logs"][name] = list(be.doc_log)
        res["spans"][name] = list(be.span_log)
        res["piped"][name] = list(piped)
    # the span= keyword reaches exactly the live blocks of this ring rank, forward and backward
    plan = doc_blocks.parse_plan(CU_GRID, SP_GRID, B, TG)
    live = doc_blocks.SpanRingPlan(plan, TG // rd, rd, rank // ud).steps
    res["live"] = (len(live), sum(1 for x in res["spans"]["layer"] if x[0] == "fwd"), sum(1 for x in res["spans"]["layer"] if x[0] == "bwd"))
    res["above"] = any(((rank // ud) - s) % rd > rank // ud for s in live)
    # the async layer: spans that are off are the call without the keyword, real ones are refused (below)
    al = Y.AsyncLongContextAttention(ring_impl_type="basic")
    a0, a1 = al(*loc[:3], causal=True), al(*loc[:3], causal=True, bidirectional=[(5, 6)])
    res["async_off"] = bool(torch.equal(a0, a1))
    lq, lk, lv2 = leaves()
    qkv = torch.stack([lq, lk.repeat_interleave(HQ // HKV, dim=2), lv2.repeat_interleave(HQ // HKV, dim=2)], dim=2)
    out = Y.LongContextAttentionQKVPacked(ring_impl_type="basic")(qkv, causal=True, cu_doclens=CU_GRID, bidirectional=SP_GRID)
    res["cases"]["qkvpacked"] = _grads(out, (lq, lk, lv2), loc[3])
    if rd == 1:
        lv = leaves()
        res["cases"]["ulysses"] = _grads(Y.UlyssesAttention(dist.group.WORLD)(*lv, causal=True, cu_doclens=CU_GRID, bidirectional=SP_GRID), lv, loc[3])
    if ud == 1:
        lv = leaves()
        res["cases"]["ring_func"] = _grads(ring_flash_attn_func(*lv, causal=True, cu_doclens=CU_GRID, bidirectional=SP_GRID,
                                                                group=Y.PROCESS_GROUP.RING_PG), lv, loc[3])
        lv = leaves()
        out1 = ring_flash_attn_func(*lv, causal=True, cu_doclens=CU_GRID, bidirectional=SP_GRID, group=Y.PROCESS_GROUP.RING_PG)
        res["cases"]["ring_func_again"] = _grads(out1, lv, loc[3])
    refusing = [(lambda kw: Y.AsyncLongContextAttention(ring_impl_type="basic")(*loc[:3], causal=True, **kw), "LongContextAttention")]
    if rd > 1:
        refusing += [(lambda kw, impl=impl: Y.LongContextAttention(ring_impl_type=impl)(*loc[:3], causal=True, **kw), "basic ring")
                     for impl in ("zigzag", "strip")]
    for call, word in refusing:
        try:
            call(dict(cu_doclens=CU_GRID, bidirectional=SP_GRID))
            res["refused"].append(False)
        except NotImplementedError as e:
            res["refused"].append(word in str(e) and "bidirectional" in str(e))
    for extra, what in ((dict(window_size=(4, 0)), "window_size"), (dict(softcap=30.0), "softcap"), (dict(alibi_slopes=torch.rand(HQ)), "alibi_slopes"),
                        (dict(dropout_p=0.1), "dropout_p"), (dict(sinks=torch.zeros(HQ)), "sinks")):
        try:
            layer(*loc[:3], causal=True, bidirectional=SP_GRID, **extra)
            res["refused"].append(False)
        except NotImplementedError as e:
            res["refused"].append(f"bidirectional together with {what}" in str(e))
    if rd == 1 and ud == 1:
        for impl in ("zigzag", "strip"):
            lv = leaves()
            res["cases"][impl] = _grads(Y.LongContextAttention(ring_impl_type=impl)(*lv, causal=True, cu_doclens=CU_GRID, bidirectional=SP_GRID),
                                        lv, loc[3])
    return res


@pytest.mark.parametrize("ud,rd", [(1, 1), (1, 2), (1, 4), (2, 2), (4, 1)], ids=lambda v: str(v))
def test_grids_against_the_unsharded_truth(ud, rd):
    import yunchang_amd as Y
    ws = ud * rd
    res = run_distributed(_worker, ws, ud, rd)
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    for rank in range(ws):
        truth = [ext(t, rank, world_size=ws, rd=rd, ud=ud) for t in _truth()]
        R = res[rank]
        for name, got in R["cases"].items():
            if name in ("none", "off_empty", "off_len1", "doc", "doc_off"):
                continue
            for g, want, what in zip(got, truth, ("out", "dq", "dk", "dv")):
                tol = TOL["bfloat16"]["out"] if what == "out" else grad_tol("bfloat16", HQ // HKV)
                assert_close(g, want, *tol, f"grid {ud}x{rd} rank {rank} {name} {what}")
        # spans that are off are the call without the keyword: the same launches, none carrying span arrays, the same bits,
        # the same exchange (with a Ulysses degree: the packed head-group exchange) -- with and without cu_doclens
        for off, base in (("off_empty", "none"), ("off_len1", "none"), ("doc_off", "doc")):
            assert R["logs"][off] == R["logs"][base] and R["spans"][off] == R["spans"][base] == []
            assert all(np.array_equal(a, b) for a, b in zip(R["cases"][off], R["cases"][base]))
            assert R["piped"][off] == R["piped"][base]
        assert (len(R["piped"]["none"]) == 1) == (ud > 1) and R["piped"]["layer"] == [] and R["piped"]["doc"] == []
        assert R["async_off"]
        # under spans every launch carries span= and none is causal; exactly the live blocks are launched
        assert R["spans"]["layer"] and all(not x[3] for x in R["spans"]["layer"])
        assert R["live"][0] == R["live"][1] == R["live"][2], R["live"]
        assert R["refused"] and all(R["refused"]), R["refused"]
        if "ring_func_again" in R["cases"]:
            assert all(np.array_equal(a, b) for a, b in zip(R["cases"]["ring_func"], R["cases"]["ring_func_again"])), "call to call: the same bits"
    if rd > 1:
        assert any(res[rank]["above"] for rank in range(ws)), "a block above the diagonal was live on some rank"
