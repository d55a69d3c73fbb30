"""The document mask (cu_doclens) without a GPU: the new tile-range functions of csrc/usp_tile_range.h against an enumeration of
(row, key) pairs; the host planner (ring/doc_blocks.py) enumerated over ring degrees 1 to 4; the C ABI before any launch; the
Python surface's refusals; LongContextAttention("basic"), its QKV-packed form, UlyssesAttention and ring_flash_attn_func on gloo
grids with the fp64 oracle backend (tests/doc_ref.py) against the unsharded truth; and the sensitivity of the GPU tests' inputs:
fp64 mutants with one boundary moved by one key fail the GPU tests' comparison."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import doc_ref
import needle_inputs
from dist_util import run_distributed
from golden_util import TOL, assert_close, grad_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "long-context-attention_amd", "csrc")

# ---- 1. the tile ranges, compiled as tests/test_tile_range_cpu.py compiles the header -----------------------------------------------
SHIM = r"""
#define USP_RANGE_FN
#include "usp_tile_range.h"
/* query side: item of BM rows, waves of WAVE rows, 64-key tiles.  Per (item, wave): t0, uncut tile of the item, then per tile of
   [0, nt): live, masked (left-bound term), as the forward and the dQ kernel use them. */
int sweep_query(const int* row_lo, int Sq, int Sk, int causal, int BM, int WAVE, int* head, int* tiles) {
  const int off = Sk - Sq, T = 64;
  int n = 0;
  for (int q0 = 0; q0 < Sq; q0 += BM) {
    const int nt = usp_tiles_holding(usp_rows_key_end(q0, BM, Sq, Sk, causal, off), T);
    *head++ = usp_doc_first_key_tile(usp_doc_row_lo(row_lo, q0, Sq, Sk), nt, T);
    *head++ = usp_doc_uncut_key_tile(usp_doc_row_lo(row_lo, q0 + BM - 1, Sq, Sk), T);
    for (int qw = q0; qw < q0 + BM; qw += WAVE) {
      const int wave_end = qw < Sq ? usp_rows_key_end(qw, WAVE, Sq, Sk, causal, off) : 0;
      const int lo0 = usp_doc_row_lo(row_lo, qw, Sq, Sk), lo1 = usp_doc_row_lo(row_lo, qw + WAVE - 1, Sq, Sk);
      for (int t = 0; t < nt; ++t) {
        *tiles++ = usp_doc_key_tile_live(t * T, T, wave_end, lo0);
        *tiles++ = usp_doc_key_tile_masked(t * T, lo1);
        ++n;
      }
    }
  }
  return n;
}
/* key side: block of OWN keys, waves of WAVE keys, 64-row tiles */
int sweep_key(const int* key_hi, int Sq, int Sk, int OWN, int WAVE, int* head, int* tiles) {
  const int T = 64, nt = (Sq + T - 1) / T;
  int n = 0;
  for (int own0 = 0; own0 < Sk; own0 += OWN) {
    *head++ = usp_doc_last_row_tile(usp_doc_key_hi(key_hi, own0 + OWN - 1, Sq, Sk), nt, T);
    for (int ow = own0; ow < own0 + OWN; ow += WAVE) {
      const int h0 = usp_doc_key_hi(key_hi, ow, Sq, Sk), h1 = usp_doc_key_hi(key_hi, ow + WAVE - 1, Sq, Sk);
      for (int t = 0; t < nt; ++t) {
        *tiles++ = usp_doc_row_tile_live(t * T, h1);
        *tiles++ = usp_doc_row_tile_masked(t * T, T, h0);
        ++n;
      }
    }
  }
  return n;
}
int clamp(int x, int n) { return usp_doc_clamp(x, n); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("docrange")
    src, lib = d / "shim.c", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.check_call(["gcc", "-O2", "-fno-semantic-interposition", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(lib)])
    return ctypes.CDLL(str(lib))


def _monotone_cases():
    rs = np.random.RandomState(0)
    cases = []
    for Sq, Sk in ((320, 320), (257, 257), (256, 512), (130, 449), (63, 63), (449, 300)):
        lists = [np.sort(rs.randint(0, Sk + 1, size=Sq)) for _ in range(3)]
        for e in (63, 64, 65, 127, 128, 129, 255, 256, 257):                     # one boundary on / before / after a multiple of 64
            lists.append(np.where(np.arange(Sq) >= min(e, Sq - 1), min(e, Sk), 0))
        lists += [np.zeros(Sq, dtype=np.int64), np.full(Sq, Sk)]
        cases += [(Sq, Sk, np.asarray(rl, dtype=np.int32)) for rl in lists]
    return cases


def test_tile_ranges_against_an_enumeration(shim):
    """Every answer of the usp_doc_* functions against the (row, key) pairs of the mask j >= row_lo[i] (and j <= i + Sk - Sq
    under causal), for random monotone arrays, single boundaries around multiples of 64, ragged Sq / Sk, both causal values and
    the geometries of the kernels: 256 / 128-row items with 32-row waves, the 128-key block with 32-key waves."""
    assert [shim.clamp(x, 5) for x in (-3, 0, 5, 9)] == [0, 0, 5, 5]
    T = 64
    for Sq, Sk, rl in _monotone_cases():
        kh = np.searchsorted(rl, np.arange(Sk), side="right").astype(np.int32)
        left = np.arange(Sk)[None, :] >= rl[:, None]                               # the left bound alone, valid pairs
        assert np.array_equal(left, np.arange(Sq)[:, None] < kh[None, :]), "row_lo and key_hi describe the same set"
        for causal in (0, 1):
            right = (np.arange(Sk)[None, :] <= np.arange(Sq)[:, None] + Sk - Sq) if causal else np.ones((Sq, Sk), bool)
            for BM in (256, 128):
                n_items = -(-Sq // BM)
                head = (ctypes.c_int * (2 * n_items))()
                tiles = (ctypes.c_int * (2 * n_items * (BM // 32) * (-(-Sk // T) + 1)))()
                shim.sweep_query(rl.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), Sq, Sk, causal, BM, 32, head, tiles)
                it = iter(tiles)
                for qi, q0 in enumerate(range(0, Sq, BM)):
                    rows = slice(q0, min(q0 + BM, Sq))
                    e = min(Sk, rows.stop + Sk - Sq) if causal else Sk
                    nt = -(-e // T) if e > 0 else 0
                    t0, unc = head[2 * qi], head[2 * qi + 1]
                    assert 0 <= t0 <= nt and not left[q0:q0 + 1, :t0 * T].any(), "no tile below t0 holds a key row q0 sees"
                    assert t0 == nt or t0 * T + T > rl[q0], "t0 is exact for the first row"
                    assert left[rows, unc * T:].all() and (unc == 0 or not left[rows, :unc * T].all()), "the uncut tile is exact"
                    for qw in range(q0, q0 + BM, 32):
                        wr = slice(qw, min(qw + 32, Sq))
                        for t in range(nt):
                            live, masked = next(it), next(it)
                            if qw >= Sq:
                                assert not live
                                continue
                            ks = slice(t * T, min(t * T + T, Sk))
                            vis = (left[wr, ks] & right[wr, ks]).any()
                            assert live or not vis, "a tile with a visible pair is live"
                            # conservative: each bound alone leaves the wave a pair, the tile taken whole (keys past Sk count)
                            assert live == bool(right[wr, ks].any() and t * T + T - 1 >= rl[qw]), "live"
                            assert masked == (not left[wr, ks].all()), "masked: some valid row does not see some key (exact)"
            # key side (the bound alone; the causal terms are the existing functions')
        n_blk = -(-Sk // 128)
        head = (ctypes.c_int * n_blk)()
        tiles = (ctypes.c_int * (2 * n_blk * 4 * (-(-Sq // T))))()
        shim.sweep_key(kh.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), Sq, Sk, 128, 32, head, tiles)
        it = iter(tiles)
        nt = -(-Sq // T)
        for bi, own0 in enumerate(range(0, Sk, 128)):
            ks = slice(own0, min(own0 + 128, Sk))
            assert not left[head[bi] * T:, ks].any(), "no row tile from t_end on sees a key of the block"
            assert head[bi] == 0 or left[(head[bi] - 1) * T:, ks.stop - 1].any(), "exact for the block's last key"
            for ow in range(own0, own0 + 128, 32):
                for t in range(nt):
                    live, masked = next(it), next(it)
                    if ow >= Sk:
                        continue
                    kw = slice(ow, min(ow + 32, Sk))
                    rows = slice(t * T, min(t * T + T, Sq))
                    assert live == left[rows, kw].any(), "live (this bound alone, exact)"
                    hidden = not left[rows, kw].all()
                    assert masked or not hidden, "a tile with a hidden pair is masked"
                    assert masked == hidden or rows.stop < t * T + T, "exact for a tile of valid rows"


# ---- 2. the planner ---------------------------------------------------------------------------------------------------------------
PLANNER_LISTS = {1: [0, 1, 2, 9, 10, 11, 48], 2: [0, 1, 24, 25, 48], 3: [0, 5, 16, 32, 47, 48], 4: [0, 1, 2, 3, 14, 24, 36, 48],
                 "span3": [0, 5, 41, 48]}


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_planner_enumerated(P):
    """Documents of length 1, of exactly S = 48 / P and spanning three ranks: row_lo / key_hi describe the same set, the union
    over a rank's launches is exactly the global mask, and the dropped blocks are exactly the empty ones."""
    from yunchang_amd.ring import doc_blocks
    T = 48
    S = T // P
    for cu in (PLANNER_LISTS[P], PLANNER_LISTS["span3"], [0] + [i * S for i in range(1, P + 1)]):
        if len(cu) == 2:
            continue
        truth = doc_ref.global_mask(cu, T)[0].numpy()
        docs = doc_blocks.parse(cu, 1, T)
        for r in range(P):
            got = np.zeros((S, T), dtype=bool)
            for step in range(r + 1):
                kr = r - step
                arr = doc_blocks.block_arrays(cu, r * S, S, kr * S, S)
                want = truth[r * S:(r + 1) * S, kr * S:(kr + 1) * S]
                assert (arr is None) == (not want.any()) == (not doc_blocks.ring_visible(docs, S, r, step)), (cu, r, step)
                if arr is None:
                    continue
                rl, kh = arr
                assert (np.diff(rl) >= 0).all() and (np.diff(kh) >= 0).all() and rl.dtype == kh.dtype == np.int32
                m1 = doc_ref.block_mask(rl, S, S, step == 0)[0].numpy()
                m2 = doc_ref.mask_of_key_hi(kh, S, S, step == 0)[0].numpy()
                assert np.array_equal(m1, m2) and np.array_equal(m1, want), (cu, r, step)
                got[:, kr * S:(kr + 1) * S] = m1
            assert np.array_equal(got, truth[r * S:(r + 1) * S]), (cu, r)
            assert not any(doc_blocks.ring_visible(docs, S, r, s) for s in range(r + 1, P))
    call = doc_blocks.ring_call(doc_blocks.parse([[0, 5, T], [0, T - 1, T]], 2, T), S, P, P - 1, "cpu")
    d = call.doc(0)
    assert d[0].dtype == torch.int32 and tuple(d[0].shape) == (2, S) and tuple(d[1].shape) == (2, S)


def test_parse():
    from yunchang_amd.ring import doc_blocks
    assert doc_blocks.parse(None, 2, 8) is None
    assert doc_blocks.parse([0, 8], 2, 8) is doc_blocks.SINGLE and doc_blocks.parse([[0, 8], [0, 8]], 2, 8) is doc_blocks.SINGLE
    assert doc_blocks.parse(torch.tensor([0, 3, 8]), 2, 8) == ((0, 3, 8),)
    assert doc_blocks.parse([[0, 3, 8], (0, 8)], 2, 8) == ((0, 3, 8), (0, 8))
    docs = doc_blocks.parse(np.array([0, 3, 8]), 1, 8)
    assert doc_blocks.parse(docs, 1, 8) is docs
    for bad in ([1, 8], [0, 3, 3, 8], [0, 5, 4, 8], [0, 7], [0, 9], [[0, 8], [0, 3, 8], [0, 8]], torch.tensor([0, 8], device="meta"), [0]):
        with pytest.raises(ValueError):
            doc_blocks.parse(bad, 2, 8)


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
    assert _C.USP_ATTN_DOC == 2048 == int(re.search(r"#define USP_ATTN_DOC (\d+)", txt).group(1))
    assert L.usp_attn_features() & _C.USP_ATTN_DOC
    assert L.usp_abi_version() == 7 == _C.ABI_VERSION
    assert (ctypes.sizeof(_C.UspFwdArgs), ctypes.sizeof(_C.UspBwdArgs)) == (296, 504)
    for name in ("usp_flash_fwd_doc", "usp_flash_bwd_doc"):
        assert name in _C.DOC_EXPORTS and name in _C.EXPORTS and hasattr(L, name)
        assert _C._doc_entry(name).restype is ctypes.c_int
    assert re.search(r"int usp_flash_fwd_doc\(const usp_fwd_args\* args, const int32_t\* row_lo, int64_t row_lo_stride_b, void\* stream\);", txt)
    assert re.search(r"int usp_flash_bwd_doc\(const usp_bwd_args\* args, const int32_t\* row_lo, int64_t row_lo_stride_b, "
                     r"const int32_t\* key_hi,\s+int64_t key_hi_stride_b, void\* stream\);", txt)
    assert len(re.findall(r"typedef struct", txt)) == 3


def test_abi_declines_without_launch():
    """Host memory stands in for the device pointers (the arrays included): every call below returns before anything is launched.
    The order: the argument checks every call gets; (backward) exactly one array missing for a launch that runs; a negative
    stride; then the declines."""
    _C, L = _lib()
    buf = ctypes.create_string_buffer(1 << 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    seq = (ctypes.c_int32 * 2)(0, 16)
    arr = (ctypes.c_int32 * 16)()
    ap = ctypes.cast(arr, ctypes.c_void_p)
    fwd, bwd = _C._doc_entry("usp_flash_fwd_doc"), _C._doc_entry("usp_flash_bwd_doc")
    calls = ((_C.UspFwdArgs, lambda a, sb=0: fwd(ctypes.byref(a), ap, sb, None), lambda a: L.usp_flash_fwd(ctypes.byref(a), None),
              lambda a: fwd(ctypes.byref(a), None, -5, None)),
             (_C.UspBwdArgs, lambda a, sb=0: bwd(ctypes.byref(a), ap, sb, ap, 0, None), lambda a: L.usp_flash_bwd(ctypes.byref(a), None),
              lambda a: bwd(ctypes.byref(a), None, -5, None, -5, None)))
    for cls, call, plain, null in calls:
        for flags, extra, want in ((_C.USP_ATTN_SOFTCAP, dict(softcap=30.0), -2), (_C.USP_ATTN_WINDOW, dict(window_left=4, window_right=0), -2),
                                   (_C.USP_ATTN_SHIFT, dict(mask_shift=0), -2), (_C.USP_FORCE_ROW64, {}, -2)):
            a = _args(_C, cls, addr)
            a.flags = flags
            for kk, vv in extra.items():
                setattr(a, kk, vv)
            assert call(a) == want, (cls.__name__, flags)
            assert call(a, -1) == -1, "a negative stride comes before the declines"
        a = _args(_C, cls, addr)                       # a packed batch
        a.seq_q = a.seq_k = ctypes.addressof(seq)
        if cls is _C.UspBwdArgs:
            a.total_k = 16
        assert call(a) == -2
        a = _args(_C, cls, addr)                       # the existing checks still come first
        a.flags, a.softmax_scale = _C.USP_FORCE_ROW64, 0.0
        assert call(a) == -1
        a = _args(_C, cls, addr)
        a.flags = _C.USP_FORCE_ROW64 | _C.USP_FORCE_WAVE32
        assert call(a) == -1
        # NULL arrays are the plain entry, whatever the strides: the same answer for a call both refuse ...
        for mut in (dict(softmax_scale=0.0), dict(D=48), dict(Hq=3)):
            a = _args(_C, cls, addr)
            for kk, vv in mut.items():
                setattr(a, kk, vv)
            assert null(a) == plain(a) != 0, mut
        assert L.usp_last_launch_kinds() == 0
    # backward: exactly one array missing is EINVAL -- unless the launch that reads it is skipped (then the refusals follow as ever)
    a = _args(_C, _C.UspBwdArgs, addr)
    assert bwd(ctypes.byref(a), ap, 0, None, 0, None) == -1 and bwd(ctypes.byref(a), None, 0, ap, 0, None) == -1
    a.flags = _C.USP_FORCE_ROW64 | _C.USP_BWD_SKIP_DKDV
    assert bwd(ctypes.byref(a), ap, 0, None, 0, None) == -2 and bwd(ctypes.byref(a), None, 0, ap, 0, None) == -1
    a.flags = _C.USP_FORCE_ROW64 | _C.USP_BWD_SKIP_DQ
    assert bwd(ctypes.byref(a), None, 0, ap, 0, None) == -2 and bwd(ctypes.byref(a), ap, 0, None, 0, None) == -1
    assert L.usp_last_launch_kinds() == 0


# ---- 4. the Python surface ---------------------------------------------------------------------------------------------------------
def test_python_refusals(monkeypatch):
    from yunchang_amd import _C
    from yunchang_amd.kernels import attention as KA
    from yunchang_amd.ring.ring_flash_attn_varlen import ring_flash_attn_varlen_func
    q = torch.zeros(2, 16, 4, 64, dtype=torch.bfloat16)
    cu = [0, 5, 16]
    for bad in ([1, 16], [0, 5, 5, 16], [0, 5, 12], [[0, 5, 16]] * 3, torch.tensor([0, 5, 16], device="meta")):
        for call in (lambda: KA.hip_attn_func(q, q, q, causal=True, cu_doclens=bad), lambda: KA.hip_attn_forward(q, q, q, causal=True, cu_doclens=bad)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(NotImplementedError, match="causal=True"):
        KA.hip_attn_func(q, q, q, causal=False, cu_doclens=cu)
    with pytest.raises(NotImplementedError, match="causal=True"):
        KA.hip_attn_func(q, q[:, :8], q[:, :8], causal=True, cu_doclens=cu)
    for kw, what in ((dict(window_size=(4, 0)), "window_size"), (dict(softcap=30.0), "softcap"), (dict(alibi_slopes=torch.rand(4)), "alibi_slopes"),
                     (dict(dropout_p=0.1), "dropout_p"), (dict(sinks=torch.zeros(4)), "sinks")):
        for fn in (KA.hip_attn_func, KA.hip_attn_forward):
            with pytest.raises(NotImplementedError, match=f"cu_doclens together with {what}"):
                fn(q, q, q, causal=True, cu_doclens=cu, **kw)
    with pytest.raises(NotImplementedError, match="cu_doclens together with softcap"):
        KA.get_block_backend(softcap=30.0, doc=True)
    # the wrapper: dense calls hand the per-launch arrays on and refuse a launch without them; packed ones refuse
    seen = {}

    class Rec:
        def fwd(self, *a, **kw):
            seen["fwd"] = kw

        def bwd(self, *a, **kw):
            seen["bwd"] = kw

        def merge(self):
            return "merge"
    prev = KA.set_block_backend(Rec())
    try:
        be = KA.get_block_backend(doc=True)
        be.fwd(1, doc=("rl", "kh"))
        be.bwd(2, doc=("rl", "kh"), only="dq")
        assert seen["fwd"] == {"doc": ("rl", "kh")} and seen["bwd"] == {"doc": ("rl", "kh"), "only": "dq"} and be.merge() == "merge"
        with pytest.raises(RuntimeError):
            be.fwd(1)
        for packed in (be.fwd_packed, be.bwd_packed):
            with pytest.raises(NotImplementedError, match="packed"):
                packed()
    finally:
        KA.set_block_backend(prev)
    with pytest.raises(NotImplementedError, match="LongContextAttention"):
        ring_flash_attn_varlen_func(q[0], q[0], q[0], torch.tensor([0, 16], dtype=torch.int32), 16, causal=True, cu_doclens=cu)
    # the array checks of the binding
    cpu = torch.device("cpu")
    rl, kh = torch.zeros(16, dtype=torch.int32), torch.zeros(2, 16, dtype=torch.int32)
    assert _C.doc_value(None, 2, 16, 16, cpu) is None and _C.doc_value((None, None), 2, 16, 16, cpu) is None
    assert _C.doc_value((rl, kh), 2, 16, 16, cpu) == ((rl, 0), (kh, 16))
    for bad in ((rl.long(), kh), (rl[:8], kh), (rl, kh.T), ([0] * 16, kh), (rl.to("meta"), kh)):
        with pytest.raises(ValueError):
            _C.doc_value(bad, 2, 16, 16, cpu)
    # a library without the feature bit
    L = _C.load()

    class Old:
        def __getattr__(self, name):
            return getattr(L, name)

        def usp_attn_features(self):
            return L.usp_attn_features() & ~_C.USP_ATTN_DOC
    monkeypatch.setattr(_C, "_lib", Old())
    with pytest.raises(NotImplementedError, match=r"\(USP_ATTN_DOC\): rebuild it"):
        _C._doc_entry("usp_flash_fwd_doc")


# ---- 5. gloo grids with the oracle backend -------------------------------------------------------------------------------------------
B, HQ, HKV, D, T = 2, 4, 2, 32, 96
SCALE = D ** -0.5
CU_GRID = [[0, 1, 30, 50, 96], [0, 47, 48, 49, 96]]         # crossing rank edges at every grid; one list per batch entry


def _inputs():
    g = torch.Generator().manual_seed(12)
    return [torch.randn(B, T, h, D, generator=g).to(torch.bfloat16) for h in (HQ, HKV, HKV, HQ)]


def _truth():
    q, k, v, do = _inputs()
    r = doc_ref.ref_bwd(do, q, k, v, SCALE, doc_ref.global_mask(CU_GRID, T, B), out_dtype=torch.bfloat16)
    return (r[0],) + r[2:]


def _grads(out, leaves, do):
    out.backward(do)
    return [t.detach().float().numpy() for t in (out,) + tuple(x.grad for x in leaves)]


def _worker(rank, ws, ud, rd):
    import torch.distributed as dist
    import yunchang_amd as Y
    from yunchang_amd.kernels import set_block_backend
    from yunchang_amd.ring import ring_flash_attn_func
    import yunchang_amd.hybrid.attn_layer as AL
    be = doc_ref.DocOracleBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    piped = []                                       # calls that took the packed / head-group-pipelined exchange

    class Counted:
        apply = staticmethod(lambda *a, _f=AL._AsyncUSPFunc.apply: (piped.append(a[8]), _f(*a))[1])
    AL._AsyncUSPFunc = Counted
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    loc = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in _inputs()]
    res = {"cases": {}, "refused": [], "logs": {}, "piped": {}}

    def leaves():
        return [t.detach().clone().requires_grad_(True) for t in loc[:3]]
    layer = Y.LongContextAttention(ring_impl_type="basic")
    for name, cu in (("layer", CU_GRID), ("single", [0, T]), ("single_b", [[0, T]] * B), ("none", None)):
        del be.doc_log[:], piped[:]
        lv = leaves()
        res["cases"][name] = _grads(layer(*lv, causal=True, cu_doclens=cu), lv, loc[3])
        res["logs"][name] = list(be.doc_log)
        res["piped"][name] = list(piped)
    # the async layer: the single document is the call without the keyword, a real mask is refused (below)
    al = Y.AsyncLongContextAttention(ring_impl_type="basic")
    a0, a1 = al(*loc[:3], causal=True), al(*loc[:3], causal=True, cu_doclens=[0, T])
    res["async_single"] = bool(torch.equal(a0, a1))
    # the QKV-packed layer: equal head counts (k, v repeated to the query heads; their gradients summed back by autograd)
    lq, lk, lv2 = leaves()
    qkv = torch.stack([lq, lk.repeat_interleave(HQ // HKV, dim=2), lv2.repeat_interleave(HQ // HKV, dim=2)], dim=2)
    out = Y.LongContextAttentionQKVPacked(ring_impl_type="basic")(qkv, causal=True, cu_doclens=CU_GRID)
    res["cases"]["qkvpacked"] = _grads(out, (lq, lk, lv2), loc[3])
    if rd == 1:
        lv = leaves()
        res["cases"]["ulysses"] = _grads(Y.UlyssesAttention(dist.group.WORLD)(*lv, causal=True, cu_doclens=CU_GRID), lv, loc[3])
    if ud == 1:
        lv = leaves()
        res["cases"]["ring_func"] = _grads(ring_flash_attn_func(*lv, causal=True, cu_doclens=CU_GRID, group=Y.PROCESS_GROUP.RING_PG), lv, loc[3])
    refusing = [(Y.AsyncLongContextAttention(ring_impl_type="basic"), "LongContextAttention")]
    if rd > 1:
        refusing += [(Y.LongContextAttention(ring_impl_type="zigzag"), "basic"), (Y.LongContextAttention(ring_impl_type="strip"), "basic")]
    for lay, word in refusing:
        try:
            lay(*loc[:3], causal=True, cu_doclens=CU_GRID)
            res["refused"].append(False)
        except NotImplementedError as e:
            res["refused"].append(word in str(e))
    if rd == 1 and ud == 1:
        for impl in ("zigzag", "strip"):
            lv = leaves()
            res["cases"][impl] = _grads(Y.LongContextAttention(ring_impl_type=impl)(*lv, causal=True, cu_doclens=CU_GRID), lv, loc[3])
    return res


@pytest.mark.parametrize("ud,rd", [(1, 1), (1, 2), (1, 4), (2, 2), (4, 1)], ids=lambda v: str(v))
def test_grids_against_the_unsharded_truth(ud, rd):
    import yunchang_amd as Y
    ws = ud * rd
    res = run_distributed(_worker, ws, ud, rd)
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    for rank in range(ws):
        truth = [ext(t, rank, world_size=ws, rd=rd, ud=ud) for t in _truth()]
        for name, got in res[rank]["cases"].items():
            if name in ("single", "single_b", "none"):
                continue
            for g, want, what in zip(got, truth, ("out", "dq", "dk", "dv")):
                tol = TOL["bfloat16"]["out"] if what == "out" else grad_tol("bfloat16", HQ // HKV)
                assert_close(g, want, *tol, f"grid {ud}x{rd} rank {rank} {name} {what}")
        # the single-document list is the call without it: the same launches, none carrying arrays, the same numbers
        for single in ("single", "single_b"):
            assert res[rank]["logs"][single] == res[rank]["logs"]["none"] and not any(x[4] for x in res[rank]["logs"]["none"])
            assert all(np.array_equal(a, b) for a, b in zip(res[rank]["cases"][single], res[rank]["cases"]["none"]))
            # ... and the same exchange: with a Ulysses degree the call without the keyword takes the packed exchange
            # (_AsyncUSPFunc, with its cap on head groups), and so does the single document; a real mask takes three exchanges
            assert res[rank]["piped"][single] == res[rank]["piped"]["none"]
        assert (len(res[rank]["piped"]["none"]) == 1) == (ud > 1) and res[rank]["piped"]["layer"] == []
        assert res[rank]["async_single"]
        assert all(x[4] for x in res[rank]["logs"]["layer"]) and res[rank]["logs"]["layer"]
        assert res[rank]["refused"] and all(res[rank]["refused"]), res[rank]["refused"]


# ---- 6. sensitivity: the GPU tests' inputs see one boundary moved by one key ----------------------------------------------------------
@pytest.mark.parametrize("S,D,dt,Hq,Hkv", [(320, 64, "bfloat16", 4, 1), (320, 32, "bfloat16", 4, 1), (1280, 128, "bfloat16", 4, 1),
                                           (320, 128, "float16", 4, 1), (320, 64, "float16", 1, 1), (320, 64, "bfloat16", 4, 4)],
                         ids=lambda v: str(v))
def test_boundary_mutants_fail(S, D, dt, Hq, Hkv):
    """On the inputs of tests/test_gpu_doc_mask.py (needle_inputs.make with doc_ref.needle_edges; both 16-bit types and the head
    layouts of its parity cases), an fp64 reference with ONE boundary moved by ONE key, in each direction, fails the GPU tests'
    comparison (golden_util.TOL for out, grad_tol for every gradient) in out, dq, dk and dv.  The check is the loop's inner
    assertion; the count below says that it ran for 100 % of the boundaries of the list, twice each."""
    from test_gpu_doc_mask import CU
    cu = CU[S]
    nd = needle_inputs.make(S, S, Hq, Hkv, D, dt, C=8, seed=S + D, edges=doc_ref.needle_edges(cu, S))
    q, k, v, do = (torch.from_numpy(x.astype(np.float32)).to(getattr(torch, dt)) for x in (nd.q, nd.k, nd.v, nd.do))
    scale = D ** -0.5
    true = doc_ref.ref_bwd(do, q, k, v, scale, doc_ref.global_mask(cu, S), out_dtype=q.dtype)
    failed = 0
    boundaries = cu[1:-1]
    for e in boundaries:
        for move in (-1, +1):
            if not (cu[cu.index(e) - 1] < e + move < cu[cu.index(e) + 1]):
                # a neighbour of length 1: moving the boundary onto the next one merges two documents -- still a wrong mask
                mut = [x for x in cu if x != e]
            else:
                mut = [e + move if x == e else x for x in cu]
            wrong = doc_ref.ref_bwd(do, q, k, v, scale, doc_ref.global_mask(mut, S), out_dtype=q.dtype)
            for name, a, b, tol in (("out", wrong[0], true[0], TOL[dt]["out"]), ("dq", wrong[2], true[2], grad_tol(dt, Hq // Hkv)),
                                    ("dk", wrong[3], true[3], grad_tol(dt, Hq // Hkv)), ("dv", wrong[4], true[4], grad_tol(dt, Hq // Hkv))):
                ok, ratio = needle_inputs.bound_ratio(a.numpy(), b.numpy(), *tol)
                assert not ok and ratio > 1.0, f"S{S} D{D}: boundary {e} moved by {move} passes in {name} (worst err / bound {ratio:.2f})"
            failed += 1
    assert failed == 2 * len(boundaries), "every boundary's two mutants were judged, and failed in all four tensors"


@pytest.mark.parametrize("dt,D", [("bfloat16", 128), ("float16", 64), ("bfloat16", 32)], ids=lambda v: str(v))
def test_offdiagonal_mutants_fail(dt, D):
    """The same for the inputs of the GPU file's full-block cases (test_gpu_doc_mask.offdiag_inputs: 256 rows against 512 earlier
    keys).  Two boundaries reach into that block: 449, the left bound of its rows 0..7, and 520, behind which rows see nothing.
    Each moved by one, in each direction, fails out, dq, dk and dv at the GPU tests' tolerances."""
    from test_gpu_doc_mask import OFFDIAG_CU, OFFDIAG_ROW0, offdiag_inputs
    from yunchang_amd.ring import doc_blocks
    nd = offdiag_inputs(dt, D)
    q, k, v, do = (torch.from_numpy(x.astype(np.float32)).to(getattr(torch, dt)) for x in (nd.q, nd.k, nd.v, nd.do))
    Sq, Sk, scale = q.shape[1], k.shape[1], D ** -0.5

    def ref(cu):
        rl, _ = doc_blocks.block_arrays(cu, OFFDIAG_ROW0, Sq, 0, Sk)
        return doc_ref.ref_bwd(do, q, k, v, scale, doc_ref.block_mask(rl, Sq, Sk, False), out_dtype=q.dtype)
    true = ref(OFFDIAG_CU)
    failed = 0
    for e in (449, 520):
        for move in (-1, +1):
            wrong = ref([e + move if x == e else x for x in OFFDIAG_CU])
            for name, a, b, tol in (("out", wrong[0], true[0], TOL[dt]["out"]), ("dq", wrong[2], true[2], grad_tol(dt, 4)),
                                    ("dk", wrong[3], true[3], grad_tol(dt, 4)), ("dv", wrong[4], true[4], grad_tol(dt, 4))):
                ok, ratio = needle_inputs.bound_ratio(a.numpy(), b.numpy(), *tol)
                assert not ok and ratio > 1.0, f"{dt} D{D}: boundary {e} moved by {move} passes in {name} (worst err / bound {ratio:.2f})"
            failed += 1
    assert failed == 4
