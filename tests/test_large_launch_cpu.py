"""CPU checks of what tests/test_gpu_large_launch.py stands on: the torch fp64 reference (tests/attn_ref_torch.py) against
the numpy oracles, the device path of the one comparator against its numpy path, and the coverage of the large-launch
table: which item walks (usp_item_deal.h) its forward and dQ launches take."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import attn_ref_torch as R
import test_softcap_cpu as SC
from golden_util import assert_close, close_mask, long_sum_atol, round_to
from oracle import usp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(B, Sq, Sk, Hq, Hkv, D, seed):
    rs = np.random.RandomState(seed)
    return [round_to(rs.standard_normal(s).astype(np.float32), "bfloat16")
            for s in [(B, Sq, Hq, D), (B, Sk, Hkv, D), (B, Sk, Hkv, D), (B, Sq, Hq, D)]]


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16)


# (B, Sq, Sk, Hq, Hkv, D, causal, window, softcap): GQA, Sq < Sk and Sq > Sk (rows without a visible key), the left-only,
# right-only and both-sided windows, softcap alone and with a window
REF_CASES = [
    (2, 40, 40, 4, 2, 16, True, None, None),
    (1, 24, 70, 6, 2, 32, True, None, None),
    (1, 70, 24, 4, 1, 16, True, None, None),
    (1, 33, 47, 2, 2, 16, False, None, None),
    (1, 50, 50, 4, 2, 16, False, (7, -1), None),
    (1, 50, 61, 4, 2, 16, False, (-1, 5), None),
    (2, 45, 38, 4, 4, 16, False, (6, 3), None),
    (1, 60, 30, 2, 1, 16, True, (9, 4), None),
    (1, 40, 56, 8, 2, 16, True, None, 2.5),
    (1, 48, 48, 4, 2, 32, False, (10, 2), 3.0),
    (1, 64, 20, 4, 2, 16, False, (3, -1), 1.5),
]


@pytest.mark.parametrize("chunk", [R.CHUNK_BYTES, 3000])
@pytest.mark.parametrize("B,Sq,Sk,Hq,Hkv,D,causal,window,cap", REF_CASES)
def test_torch_reference_matches_the_numpy_oracles(B, Sq, Sk, Hq, Hkv, D, causal, window, cap, chunk):
    """To 1e-10 against O.attention_ref / O.block_bwd (no cap) and test_softcap_cpu.ref_fwd / ref_bwd_from (window and
    cap), in one chunk and in chunks of a few rows (chunk = 3000 bytes: every chunk reads its own key range)."""
    q, k, v, do = _case(B, Sq, Sk, Hq, Hkv, D, seed=Sq * 7 + Sk)
    scale = D ** -0.5
    tq, tk, tv, tdo = (_t(x) for x in (q, k, v, do))
    ro, rl = R.ref_fwd(tq, tk, tv, scale, causal, window, cap, chunk_bytes=chunk)
    if cap is None:
        wo, wl = O.attention_ref(q, k, v, causal, scale, window=window or (-1, -1))
    else:
        wo, wl = SC.ref_fwd(q, k, v, scale, cap, causal, window)
    assert ro.dtype == torch.float64 and rl.dtype == torch.float64
    empty = ~np.isfinite(wl)
    if causal and Sq > Sk:
        assert empty.any()                                      # the case has rows without a visible key
    assert_close(rl, wl, 1e-10, 1e-10, "lse")                   # (-inf == -inf passes; anything else at -inf fails)
    assert_close(ro, wo, 1e-10, 1e-10, "out")
    assert bool((ro.permute(0, 2, 1, 3)[torch.from_numpy(empty)] == 0).all())
    o16 = ro.to(torch.bfloat16)
    o16n = o16.double().numpy()
    dq, dk, dv, delta = R.ref_bwd(tdo, tq, tk, tv, o16, rl, scale, causal, window, cap, chunk_bytes=chunk)
    if cap is None:
        want = O.block_bwd(do, q, k, v, o16n, wl, scale, causal, window=window or (-1, -1))
    else:
        wdelta = np.einsum("bshd,bshd->bhs", do.astype(np.float64), o16n)
        assert_close(delta, wdelta, 1e-10, 1e-10, "delta")
        want = SC.ref_bwd_from(do, q, k, v, wl, wdelta, scale, cap, causal, window)
    for g_, w_, n_ in zip((dq, dk, dv), want, ("dq", "dk", "dv")):
        assert_close(g_, w_, 1e-10, 1e-10, n_)
    assert bool((dq.permute(0, 2, 1, 3)[torch.from_numpy(empty)] == 0).all())


def test_reference_chunks_cover_every_row_once_and_only_visible_keys():
    for Sq, Sk, Hq, causal, window in [(1000, 1000, 4, True, None), (700, 300, 2, True, None), (300, 900, 8, False, (50, 0)),
                                       (513, 513, 3, False, (-1, 17)), (64, 64, 1, False, None)]:
        left, right, off = R._bounds(Sq, Sk, causal, window)
        vis = SC._mask(Sq, Sk, causal, window)
        for budget in (8 * Hq * 100, 8 * Hq * 5000, R.CHUNK_BYTES):
            rows = []
            for r0, r1, k0, k1 in R._chunks(Sq, Sk, Hq, left, right, off, budget):
                rows.extend(range(r0, r1))
                assert (r1 - r0) == 1 or 8 * Hq * (r1 - r0) * (k1 - k0) <= budget
                sub = vis[r0:r1]
                assert not sub[:, :k0].any() and not sub[:, k1:].any()    # nothing visible outside the key range
            assert rows == list(range(Sq))


# ---- the one comparator, on the device path and on the numpy path ---------------------------------------------------
_CRAFTED = [
    ([1.0, -np.inf, 2.0], [1.0, -np.inf, 2.0]),
    ([np.nan, -np.inf, 2.0], [1.0, -np.inf, 2.0]),
    ([1.0, np.inf, 2.0], [1.0, -np.inf, 2.0]),
    ([1.0, np.nan, 2.0], [1.0, -np.inf, 2.0]),
    ([1.0, -np.inf, 3.0], [1.0, -np.inf, 2.0]),
    ([1.0, 5.0, 2.0], [1.0, np.inf, 2.0]),
    ([np.inf, np.inf, -np.inf], [np.inf, np.inf, -np.inf]),
    ([1.0, 2.0, 3.0], [1.0, 2.0, np.nan]),
    ([1.0005, -2.001, 0.0], [1.0, -2.0, 1e-3]),
    ([1.0015, -2.001, 0.0], [1.0, -2.0, 1e-3]),
]


@pytest.mark.parametrize("got,want", _CRAFTED)
def test_comparator_torch_and_numpy_paths_agree(got, want):
    """Same verdict element by element (NaN never passes, the identical infinity does), same error values and the same
    message, whether the operands are numpy arrays, torch tensors or one of each."""
    g, w = np.array(got), np.array(want)
    ok_np, err_np = close_mask(g, w, 1e-3, 0.0)
    try:
        assert_close(g, w, 1e-3, 0.0, "x")
        msg_np = None
    except AssertionError as e:
        msg_np = str(e)
    assert (msg_np is None) == bool(ok_np.all())
    for tg, tw in ((torch.tensor(g), torch.tensor(w)), (torch.tensor(g), w), (g, torch.tensor(w))):
        ok_t, err_t = close_mask(tg, tw, 1e-3, 0.0)
        assert isinstance(ok_t, torch.Tensor) and ok_t.dtype == torch.bool
        assert np.array_equal(ok_t.numpy(), ok_np)
        assert np.array_equal(err_t.numpy(), err_np, equal_nan=True)
        try:
            assert_close(tg, tw, 1e-3, 0.0, "x")
            msg_t = None
        except AssertionError as e:
            msg_t = str(e)
        assert msg_t == msg_np


def test_comparator_message_form_on_the_device_path():
    w = torch.zeros(2, 3, 4, dtype=torch.float64)
    g = w.clone()
    g[1, 2, 3] = 0.5
    g[0, 1, 0] = float("nan")
    with pytest.raises(AssertionError) as e:
        assert_close(g, w, 1e-3, 1e-3, "what")
    assert str(e.value).startswith("what: 2 / 24 elements out of tolerance (atol=0.001, rtol=0.001); 1 NaN in the result; "
                                   "max finite abs err 5.000e-01 at ")
    assert str(e.value).endswith(f"at {np.unravel_index(23, (2, 3, 4))}; first bad element at {np.unravel_index(4, (2, 3, 4))}")
    with pytest.raises(AssertionError) as e2:
        assert_close(g.numpy(), w.numpy(), 1e-3, 1e-3, "what")
    assert str(e2.value) == str(e.value)


def test_long_sum_floor_is_one_rule():
    """golden_util.long_sum_atol is the rule test_gpu_fuzz and test_gpu_row64 applied in place, bit for bit (numpy), and
    the device path gives the same bound to the last few ulps."""
    rs = np.random.RandomState(0)
    r = rs.standard_normal((3, 50, 4, 8)) * 7.0
    old = max(5e-2, 8e-3 * float(np.sqrt(np.mean(np.square(r, dtype=np.float64)))))
    assert long_sum_atol(5e-2, 1000, r) == old
    assert long_sum_atol(5e-2, 999, r) == 5e-2
    assert long_sum_atol(5e-2, 4000, r * 1e-3) == 5e-2
    assert abs(long_sum_atol(5e-2, 1000, torch.from_numpy(r)) - old) <= 1e-15 * old


# ---- coverage of the large-launch table: the item walks of its forward and dQ launches -----------------------------
@pytest.fixture(scope="module")
def walk_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("deal")
    src = d / "deal.c"
    src.write_text('#define USP_DEAL_FN\n#include "usp_item_deal.h"\n')
    lib = d / "libdeal.so"
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "long-context-attention_amd", "csrc"), str(src), "-o", str(lib)])
    L = ctypes.CDLL(str(lib))
    L.usp_deal_item.restype = L.usp_group_item.restype = ctypes.c_int
    return L


def _walk(L, n_items, slots, n_inner, G, grouped):
    """What ItemWalk (usp_common.hpp) hands out over all workgroups of a persistent launch: (decoded ids in walk order,
    items per run, dealt?, grouped?)."""
    grid = slots if n_items > slots else n_items
    by_xcd = grid % 8 == 0 and n_items % 8 == 0
    items_l = n_items // 8 if by_xcd else n_items
    wgs_l = grid // 8 if by_xcd else grid
    ids, dealt, walked = [], False, False
    for x in range(8 if by_xcd else 1):
        for wg in range(wgs_l):
            p = 0
            while True:
                loc = p * wgs_l + ((wgs_l - 1 - wg) if p & 1 else wg)
                if loc >= items_l:
                    break
                w = x * items_l + loc
                d = L.usp_deal_item(w, n_inner, items_l)
                g = L.usp_group_item(d, n_inner, items_l, G) if grouped else d
                dealt |= d != w
                walked |= g != d
                ids.append(g)
                p += 1
    return ids, items_l, dealt, walked


def test_large_launch_table_reaches_every_item_walk(walk_lib):
    import test_gpu_large_launch as LL
    seen = set()
    for case in LL.CASES:
        G = case.Hq // case.Hkv
        fk, fn, fslots, f_inner, fks = LL.fwd_launch(case)
        qk, qn, qslots, q_inner, qks = LL.dq_launch(case)
        launches = [(fk, fn, fslots, f_inner, fk == "fwd_row64" and fks == 1),
                    (qk, qn, qslots, q_inner, qk == "dq_row64" and qks == 1)]
        for kind, n, slots, n_inner, grouped in launches:
            assert n > slots, (case.id, kind, n, slots)
            ids, items_l, dealt, walked = _walk(walk_lib, n, slots, n_inner, G, grouped)
            assert sorted(ids) == list(range(n)), (case.id, kind)       # every item exactly once
            if dealt:
                seen.add("regular dealing" if n_inner % items_l == 0 else "irregular dealing")
            if walked:
                seen.add("group walk")
            if n % 8:
                seen.add("count not divisible by 8")
    assert seen == {"regular dealing", "irregular dealing", "group walk", "count not divisible by 8"}, seen


def test_large_launch_table_is_multi_pass_and_names_its_kernels():
    """Every default case: each flash launch has more items than resident workgroups (256 CUs), the declared kinds are
    consistent with the shape (K split / cuts / head split), and every row of the issue's table has a default case."""
    import test_gpu_large_launch as LL
    kinds = set()
    for case in LL.CASES:
        _, fn, fslots, _, _ = LL.fwd_launch(case)
        _, qn, qslots, _, _ = LL.dq_launch(case)
        _, kn, kslots = LL.dkdv_launch(case)
        assert fn > fslots and qn > qslots and kn > kslots, case.id
        kinds |= set(case.fwd) | set(case.bwd)
    assert kinds == set(__import__("yunchang_amd")._C.KINDS.values()), kinds
    assert [c.id for c in LL.CASES] == ["A", "B", "C", "D", "E", "E2", "F", "G", "H", "I", "J", "K", "L"]
