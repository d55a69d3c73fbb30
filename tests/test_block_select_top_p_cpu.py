"""Top-p block selection (`block_select=BlockSelectTopP(...)`) without a GPU: the fp64 reference (tests/block_select_top_p_ref.py)
against a brute-force enumeration and under its own acceptance rule, mutants of the reference that must fail the rule on the
inputs the GPU tests use, how often those inputs are ambiguous (judged on the reference and the derived bounds alone), the
argument logic and refusals of the Python layers, and the rings and layers on gloo with an fp64 backend
(tests/block_select_top_p_backend.py)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import block_mask_ref as BR
import block_select_inputs as X
import block_select_ref as SR
import block_select_top_p_inputs as TX
import block_select_top_p_ref as TR
from golden_util import TOL, assert_close, grad_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the reference against a brute-force enumeration, and under its own rule -----------------------------------------------------
def brute(q, k, top_p, scale, causal, keep_first, keep_local, share):
    B, S, Hq, D = q.shape
    Hkv, nb = k.shape[2], (S + 127) // 128
    G = Hq // Hkv
    qn, kn = q.double().numpy(), k.double().numpy()
    out = np.zeros((B, Hq, nb, nb), dtype=bool)
    mean = lambda x, b, blk, h: x[b, blk * 128:min(S, (blk + 1) * 128), h].sum(axis=0) / (min(S, (blk + 1) * 128) - blk * 128)

    def head_weights(b, h, I, vis):
        sc = np.array([scale * float(mean(qn, b, I, h) @ mean(kn, b, J, h // G)) for J in vis])
        e = np.exp(sc - sc.max())
        return e / e.sum()
    for b in range(B):
        for h in range(Hq):
            for I in range(nb):
                vis = [J for J in range(nb) if not causal or J <= I]
                if share:
                    g0 = (h // G) * G
                    w = sum(head_weights(b, g, I, vis) for g in range(g0, g0 + G)) / G
                else:
                    w = head_weights(b, h, I, vis)
                w = dict(zip(vis, w))
                forced = [J for J in vis if J < keep_first or I - keep_local < J <= I]
                rest = sorted((J for J in vis if J not in forced), key=lambda J: (-w[J], J))
                mass, chosen = sum(w[J] for J in forced), []
                for J in rest:
                    if mass >= top_p:
                        break
                    chosen.append(J)
                    mass += w[J]
                out[b, h, I, forced + chosen] = True
    return torch.from_numpy(out)


@pytest.mark.parametrize("S,Hq,Hkv,D", [(300, 2, 1, 8), (640, 4, 2, 16), (129, 2, 2, 8)])
def test_reference_matches_brute_force(S, Hq, Hkv, D):
    q, k = X.white(2, S, Hq, Hkv, D, torch.bfloat16, seed=S)
    for causal in (True, False):
        for top_p in (0.05, 0.4, 0.75, 0.97):
            for kf, kl in ((0, 1), (2, 2), (1, 0)):
                if causal and kl < 1:
                    continue
                for share in (False, True):
                    got = TR.select_ref(q, k, top_p, 3.7, causal, kf, kl, share)
                    assert torch.equal(got, brute(q, k, top_p, 3.7, causal, kf, kl, share)), (causal, top_p, kf, kl, share)


def test_group_of_one_is_the_unshared_selection():
    q, k = X.white(1, 640, 3, 3, 16, torch.bfloat16, seed=4)
    for causal in (True, False):
        assert torch.equal(TR.select_ref(q, k, 0.6, 2.0, causal, 1, 1, True), TR.select_ref(q, k, 0.6, 2.0, causal, 1, 1, False))


def _white_problem(case):
    S, Hq, Hkv, D, dtype, seed = case
    q, k = X.white(1, S, Hq, Hkv, D, dtype, seed)
    return q, k, TR.Problem(q, k)


# ---- 2. the ambiguity cap: a condition on the inputs, from the reference and the derived bounds alone ----------------------------------
@pytest.mark.parametrize("case", X.WHITE_CASES, ids=lambda c: f"S{c[0]}")
def test_white_cases_pass_their_own_rule_and_are_rarely_ambiguous(case):
    q, k, prob = _white_problem(case)
    judged = [prob.judge(p, causal, kf, kl, share) for causal, kf, kl, p, share in TX.white_grid()]
    for j in judged:
        assert bool(j.passes(j.mask).all())
    share = TX.case_ambiguity(judged)
    print(f"AMBIGUOUS white S={case[0]} D={case[3]}: {share:.5f} of the rows, largest E {max(float(j.E.max()) for j in judged):.3e}")
    assert share <= TX.CAP


@pytest.mark.parametrize("nbk", TX.SYNTH_NBK)
def test_synthetic_cases_pass_their_own_rule_are_rarely_ambiguous_and_spread_the_counts(nbk):
    qbar, kbar = TX.synthetic_means(nbk)
    peaked = TX.peaked_scale(qbar, kbar)
    assert peaked > TX.SYNTH_D ** -0.5
    for scale in (TX.SYNTH_D ** -0.5, peaked):
        prob = TR.Problem(scale=scale, means=(qbar, kbar))
        judged = [prob.judge(p, causal, kf, kl, share, row0) for causal, row0, kf, kl, p, share in TX.synth_grid(nbk)]
        for j in judged:
            assert bool(j.passes(j.mask).all())
        share = TX.case_ambiguity(judged)
        print(f"AMBIGUOUS synthetic nbk={nbk} scale={scale:.4f}: {share:.5f} of the rows")
        assert share <= TX.CAP
    if nbk >= 5:        # at the peaked scale the counts run from one block to most of what a row sees
        lo, _ = prob.judge(0.05, False, 0, 0).counts()
        hi, vis = prob.judge(0.9, False, 0, 0).counts()
        assert int(lo.min()) == 1 and float((hi.double() / vis).max()) >= 0.7
        flat = TR.Problem(scale=TX.SYNTH_D ** -0.5, means=(qbar, kbar)).judge(0.9, False, 0, 0)
        assert float(flat.w[0, 0, 0].max() / flat.w[0, 0, 0].min()) < 1.25, "row 0 is nearly uniform at the default scale"


# ---- 3. mutants --------------------------------------------------------------------------------------------------------------------------
def test_mutants_fail():
    """Each fp64 mutant must fail the rule the GPU tests apply, on inputs the GPU tests use; the unmutated reference passes."""
    seen = set()
    # planted rankings (tests/block_select_inputs.py: PLANTED_CASES[2], [3]); white noise where the mutant moves whole weights
    q, k, _, _ = X.planted(1, 1024, 8, 1, 32, torch.bfloat16, 3)
    prob = TR.Problem(q, k, TX.PLANTED_SCALE)
    for name, (p, causal, kf, kl, share) in (("mass_without_forced", (0.5, True, 1, 2, False)),
                                             ("softmax_all_blocks", (0.5, True, 0, 1, False)),
                                             ("count_share", (0.5, False, 0, 1, False)),
                                             ("one_short", (0.5, False, 0, 1, False)),
                                             ("one_long", (0.5, False, 0, 1, False)),
                                             ("share_avg_scores", (0.5, True, 0, 1, True)),
                                             ("share_unnormalised", (0.5, True, 0, 1, True))):
        j = prob.judge(p, causal, kf, kl, share)
        assert TR.agrees(TR.select_ref(q, k, p, TX.PLANTED_SCALE, causal, kf, kl, share), j), name
        assert not TR.agrees(TR.select_ref(q, k, p, TX.PLANTED_SCALE, causal, kf, kl, share, mutant=name), j), name
        seen.add(name)
    q, k, _, _ = X.planted(1, 4400, 4, 2, 64, torch.bfloat16, 4)
    prob = TR.Problem(q, k)
    j = prob.judge(0.5, False, 0, 1)
    assert TR.agrees(TR.select_ref(q, k, 0.5), j)
    assert not TR.agrees(TR.select_ref(q, k, 0.5, mutant="wrong_kv_head"), j)
    seen.add("wrong_kv_head")
    # the white cases too: a mutant that passes there would not be seen by the end-to-end GPU tests
    q, k, prob = _white_problem(X.WHITE_CASES[4])
    for name, share in (("mass_without_forced", False), ("softmax_all_blocks", False), ("count_share", False), ("one_short", False),
                        ("one_long", False), ("wrong_kv_head", False)):     # (the two share_group mutants move white-noise weights by
        # less than eps -- nearly uniform weights average alike either way: the planted inputs at PLANTED_SCALE above see them)
        j = prob.judge(0.5, True, 0, 2, share)
        assert not TR.agrees(TR.select_ref(q, k, 0.5, None, True, 0, 2, share, mutant=name), j), name
    # the row-block offset of a ring rank: rank 1 of 2 against its rows of the whole selection
    q, k, _, _ = X.planted(1, 1024, 8, 1, 32, torch.bfloat16, 3)
    whole = TR.select_ref(q, k, 0.5, None, True, 0, 1)
    assert torch.equal(TR.select_ref_rows(q, k, 0.5, 32 ** -0.5, True, 0, 1, False, 2, 1), whole[:, :, 4:])
    assert not torch.equal(TR.select_ref_rows(q, k, 0.5, 32 ** -0.5, True, 0, 1, False, 2, 1, mutant="drop_row_offset"), whole[:, :, 4:])
    seen.add("drop_row_offset")
    # ties: on the twins the lower J must come first, and the rule's exact-tie clause sees the mutant
    q, k = X.twins(1, 1024, 4, 2, 32, 2, 5)
    prob = TR.Problem(q, k)
    hit = False
    for p in (0.2, 0.3, 0.4, 0.5, 0.6, 0.7):
        j = prob.judge(p, False, 0, 0)
        assert TR.agrees(TR.select_ref(q, k, p, None, False, 0, 0), j)
        bad = TR.select_ref(q, k, p, None, False, 0, 0, mutant="tie_high")
        if not torch.equal(bad, j.mask):
            hit = True
            assert not TR.agrees(bad, j), p
    assert hit, "no top_p of the list cuts between the twins"
    seen.add("tie_high")
    assert seen == set(TR.MUTANTS)


def test_equal_weights_select_the_lowest_blocks():
    q, k = X.zero_q(1, 1024, 4, 2, 32)
    for causal, kf, kl, p, share in TX.white_grid():
        m = TR.select_ref(q, k, p, None, causal, kf, kl, share)
        visible, forced = SR.candidates(8, 8, causal, kf, kl)
        cand = visible & ~forced
        n = (m & cand).sum(-1, keepdim=True)
        assert torch.equal(m, (forced | (cand & (cand.cumsum(-1) <= n))).expand_as(m))
        nv, nf = visible.sum(-1), forced.sum(-1)
        want = torch.tensor([0 if nf[i] / nv[i] >= p else min(int(nv[i] - nf[i]), math.ceil(float(p * nv[i] - nf[i]) - 1e-9))
                             for i in range(8)])
        assert torch.equal(n[0, 0, :, 0], want), (causal, kf, kl, p)


# ---- 4. argument logic -------------------------------------------------------------------------------------------------------------------
def test_block_select_top_p_value():
    from yunchang_amd import _C
    v = _C.block_select_top_p_value
    assert v(0.9) == (0.9, 0, 1, False) and v(1, 2, 3, True, True) == (1.0, 2, 3, True) and v(1e-9, 0, 0) == (1e-9, 0, 0, False)
    for bad in (0, 0.0, -0.1, 1.0001, 2, float("nan"), float("inf"), True, False, "0.5", None, [0.5]):
        with pytest.raises(ValueError, match="top_p"):
            v(bad)
    for kw in (dict(keep_first=-1), dict(keep_first=1.0), dict(keep_first=True), dict(keep_local=-1), dict(keep_local=1.5),
               dict(keep_local=False), dict(share_group=1), dict(share_group=None), dict(share_group="yes")):
        with pytest.raises(ValueError, match=list(kw)[0]):
            v(0.5, **kw)
    with pytest.raises(ValueError, match="keep_local >= 1"):
        v(0.5, 0, 0, False, True)
    assert v(0.5, 0, 0, False, False) == (0.5, 0, 0, False)


class Recorder:
    """A block backend that records its calls and computes nothing."""
    name = "recorder"

    def __init__(self):
        self.calls = []

    def fwd(self, q, k, v, scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None, **kw):
        self.calls.append(("fwd", causal, merge_in, kw))
        lse.zero_()
        if out is not None:
            out.zero_()

    def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, scale, causal, **kw):
        self.calls.append(("bwd", causal, kw))

    def delta(self, dout, out, delta):
        delta.zero_()

    def block_means(self, x):
        self.calls.append(("means", tuple(x.shape)))
        return torch.zeros((x.shape[0], (x.shape[1] + 127) // 128, x.shape[2], x.shape[3]))

    def block_select(self, *a, **kw):
        raise AssertionError("the top-k selection was called for a BlockSelectTopP")

    def block_select_top_p(self, qbar, kbar, top_p, scale, causal, keep_first=0, keep_local=1, share_group=False, row_block0=0):
        self.calls.append(("select_top_p", top_p, scale, causal, keep_first, keep_local, share_group, row_block0))
        return torch.ones((qbar.shape[0], qbar.shape[2], qbar.shape[1], kbar.shape[1]), dtype=torch.bool)


@pytest.fixture
def recorder():
    from yunchang_amd.kernels import attention as K
    rec = Recorder()
    prev = K.set_block_backend(rec)
    yield rec
    K.set_block_backend(prev)


def _small():
    q = torch.zeros(1, 256, 4, 32, dtype=torch.bfloat16)
    k = torch.zeros(1, 256, 2, 32, dtype=torch.bfloat16)
    return q, k, k.clone()


REFUSED = [("block_mask", dict(block_mask=torch.ones(2, 2, dtype=torch.bool))), ("window_size", dict(window_size=(64, 0))),
           ("softcap", dict(softcap=30.0)), ("alibi_slopes", dict(alibi_slopes=torch.ones(4))), ("dropout_p", dict(dropout_p=0.1)),
           ("sinks", dict(sinks=torch.zeros(4))), ("cu_doclens", dict(cu_doclens=[0, 128, 256])),
           ("bidirectional", dict(bidirectional=[(0, 8)]))]


@pytest.mark.parametrize("name,kw", REFUSED, ids=[n for n, _ in REFUSED])
def test_refusal_table(recorder, name, kw):
    """The sentences of the top-k record, for the new record alike, before any tensor is read."""
    import yunchang_amd as Y
    from yunchang_amd.kernels.attention import hip_attn_forward, hip_attn_func
    from yunchang_amd.kernels.features import block_select_alone
    from yunchang_amd.ring.ring_flash_attn import ring_flash_attn_func
    from yunchang_amd.ring.zigzag_ring_flash_attn import zigzag_ring_flash_attn_func
    q, k, v = _small()
    msg = f"block_select together with {name} is not supported by the HIP attention kernels"
    for sel in (Y.BlockSelectTopP(0.9), Y.BlockSelect(2)):
        with pytest.raises(NotImplementedError) as e:
            block_select_alone(sel, **kw)
        assert str(e.value) == msg
    for fn in (hip_attn_forward, hip_attn_func, ring_flash_attn_func, zigzag_ring_flash_attn_func):
        with pytest.raises(NotImplementedError) as e:
            fn(q, k, v, causal=True, block_select=Y.BlockSelectTopP(0.9, 1, 1, True), **kw)
        assert str(e.value) == msg
    assert recorder.calls == []


def test_other_refusals_and_value_errors(recorder):
    import yunchang_amd as Y
    from yunchang_amd.comm.all_to_all import local_options
    from yunchang_amd.hybrid.async_attn_layer import AsyncLongContextAttention
    from yunchang_amd.kernels import BlockSelectTopP as K_TopP, select_blocks_top_p as k_select
    from yunchang_amd.kernels.attention import hip_attn_forward, hip_attn_func, select_blocks_top_p
    from yunchang_amd.kernels.features import BlockSelectTopP, block_select_alone
    from yunchang_amd.ring import front_end as F
    from yunchang_amd.ring.ring_flash_attn_varlen import ring_flash_attn_varlen_func
    q, k, v = _small()
    assert Y.BlockSelectTopP is BlockSelectTopP is K_TopP and Y.select_blocks_top_p is select_blocks_top_p is k_select
    sel = Y.BlockSelectTopP(0.9)
    assert sel == (0.9, 0, 1, False) and sel._fields == ("top_p", "keep_first", "keep_local", "share_group")
    assert Y.BlockSelect(2) == (2, 0, 1), "the top-k record stays a 3-tuple"
    assert block_select_alone(sel) is True and block_select_alone(Y.BlockSelect(2)) is True and block_select_alone(None) is False
    with pytest.raises(AttributeError):
        sel.top_p = 0.5
    with pytest.raises(NotImplementedError, match="return_max_logits together with block_select"):
        hip_attn_func(q, k, v, block_select=sel, return_max_logits=True)
    with pytest.raises(NotImplementedError, match="block_select needs whole q and k of the same length"):
        hip_attn_forward(q, k[:, :128], v[:, :128], block_select=sel)
    with pytest.raises(NotImplementedError, match="same length"):
        select_blocks_top_p(q, k[:, :128], 0.9)
    for bad in ((0.9, 0, 1, False), 0.9, "0.9", [0.9]):
        with pytest.raises(ValueError, match="^block_select must be a BlockSelect\\(top_k, keep_first=0, keep_local=1\\)"):
            hip_attn_forward(q, k, v, block_select=bad)
    for bad in (Y.BlockSelectTopP(0.0), Y.BlockSelectTopP(1.5), Y.BlockSelectTopP(True), Y.BlockSelectTopP(float("nan")),
                Y.BlockSelectTopP(0.5, -1), Y.BlockSelectTopP(0.5, 0, 1.5), Y.BlockSelectTopP(0.5, 0, 1, 1)):
        with pytest.raises(ValueError):
            hip_attn_forward(q, k, v, block_select=bad)
        with pytest.raises(ValueError):
            select_blocks_top_p(q, k, bad.top_p, keep_first=bad.keep_first, keep_local=bad.keep_local, share_group=bad.share_group)
    with pytest.raises(ValueError, match="keep_local >= 1"):
        hip_attn_forward(q, k, v, causal=True, block_select=Y.BlockSelectTopP(0.9, 0, 0))
    with pytest.raises(ValueError, match="keep_local >= 1"):
        select_blocks_top_p(q, k, 0.9, causal=True, keep_local=0)
    select_blocks_top_p(q, k, 0.9, causal=False, keep_local=0)
    with pytest.raises(TypeError):
        select_blocks_top_p(q.float(), k.float(), 0.9)
    with pytest.raises(NotImplementedError, match="variable-length.*ring_flash_attn_func"):
        ring_flash_attn_varlen_func(q[0], k[0], v[0], torch.tensor([0, 256], dtype=torch.int32), 256, block_select=sel)
    with pytest.raises(NotImplementedError, match="block_select.*AsyncLongContextAttention.*LongContextAttention"):
        AsyncLongContextAttention.forward(None, q, k, v, block_select=sel)
    # share_group where a KV group is split over ulysses ranks (fewer KV heads than ranks): refused, naming it
    shared = Y.BlockSelectTopP(0.9, share_group=True)
    for kv_heads, P in ((1, 2), (2, 4), (1, 4)):
        with pytest.raises(NotImplementedError, match="share_group"):
            local_options(None, 0.0, None, None, 8, P, 0, True, "x", block_select=shared, kv_heads=kv_heads)
    for kv_heads, P in ((2, 2), (4, 2), (8, 4), (1, 1)):
        assert local_options(None, 0.0, None, None, 8, P, 0, True, "x", block_select=shared, kv_heads=kv_heads)[0] == \
            dict(block_select=shared)
    assert local_options(None, 0.0, None, None, 8, 4, 0, True, "x", block_select=sel, kv_heads=1)[0] == dict(block_select=sel)

    class G4:
        pass
    orig = F.group_info
    F.group_info = lambda dist, group: (4, 1)
    try:
        with pytest.raises(NotImplementedError, match="block_select across ring steps.*zigzag and stripe rings.*basic ring"):
            F._place_block_select(F.DENSE_RING, q, k, F.BlockSelection(sel), True, G4())
        with pytest.raises(NotImplementedError, match="block_select at ring degree 4.*multiple of 128"):
            F._place_block_select(F.BASIC_RING, q[:, :200], k[:, :200], F.BlockSelection(sel), True, G4())
        with pytest.raises(ValueError, match="keep_local >= 1"):
            F._place_block_select(F.BASIC_RING, q, k, F.BlockSelection(Y.BlockSelectTopP(0.9, 0, 0)), True, G4())
        F._place_block_select(F.BASIC_RING, q, k, F.BlockSelection(sel), True, G4())
    finally:
        F.group_info = orig


def test_one_selection_per_call_and_the_mask_goes_to_the_backward(recorder):
    import yunchang_amd as Y
    from yunchang_amd.kernels.attention import hip_attn_forward, hip_attn_func
    from yunchang_amd.ring.ring_flash_attn import ring_flash_attn_func
    q, k, v = _small()
    hip_attn_forward(q, k, v, causal=True)
    hip_attn_forward(q, k, v, causal=True, block_select=None)
    assert recorder.calls[0] == recorder.calls[1] and len(recorder.calls) == 2
    del recorder.calls[:]
    hip_attn_forward(q, k, v, causal=True, softmax_scale=0.5, block_select=Y.BlockSelectTopP(0.75, 1, 2, True))
    assert [c[0] for c in recorder.calls] == ["means", "means", "select_top_p", "fwd"]
    assert recorder.calls[2] == ("select_top_p", 0.75, 0.5, True, 1, 2, True, 0)
    assert recorder.calls[3][3]["bsp"].dtype == torch.bool
    import torch.distributed as dist
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:29793", rank=0, world_size=1)
    try:
        for fn in (hip_attn_func, lambda *a, **kw: ring_flash_attn_func(*a, group=None, **kw)):
            del recorder.calls[:]
            lq, lk, lv = (t.clone().requires_grad_(True) for t in (q, k, v))
            out = fn(lq, lk, lv, causal=True, block_select=Y.BlockSelectTopP(0.9))
            out.sum().backward()
            kinds = [c[0] for c in recorder.calls]
            assert kinds == ["means", "means", "select_top_p", "fwd", "bwd"], kinds
            assert recorder.calls[4][2]["bsp"] is recorder.calls[3][3]["bsp"]
            assert lq.grad is not None
    finally:
        if own:
            dist.destroy_process_group()


def test_padded_head_dims_select_on_the_padded_operands(recorder):
    import yunchang_amd as Y
    from yunchang_amd.kernels.attention import hip_attn_forward
    q = torch.zeros(1, 256, 4, 24, dtype=torch.bfloat16)
    k = torch.zeros(1, 256, 2, 24, dtype=torch.bfloat16)
    hip_attn_forward(q, k, k.clone(), block_select=Y.BlockSelectTopP(0.5))
    assert recorder.calls[0] == ("means", (1, 256, 4, 32)) and recorder.calls[2][2] == pytest.approx(24 ** -0.5)


# ---- 5. the C ABI surface ------------------------------------------------------------------------------------------------------------------
def test_binding_matches_the_header():
    from yunchang_amd import _C
    txt = open(os.path.join(ROOT, "include", "usp_hip.h")).read()
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
             "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    assert _C.SELECT_TOP_P_EXPORTS == ("usp_block_select_top_p",)
    proto = re.search(r"\nint usp_block_select_top_p\(([^;]*)\);", txt).group(1)
    params = [p.split() for p in proto.replace("\n", " ").split(",")]
    assert [p[-1] for p in params] == ["qbar", "kbar", "B", "Hq", "Hkv", "D", "nbq", "nbk", "row_block0", "scale", "causal", "top_p",
                                       "keep_first", "keep_local", "share_group", "mask", "mask_stride_b", "mask_stride_h",
                                       "mask_stride_row", "stream"]
    bit, _, argtypes = _C._FEATURE_ENTRIES["usp_block_select_top_p"]
    assert bit == _C.USP_ATTN_BLOCK_SELECT_TOP_P and [ctype[" ".join(p[:-1])] for p in params] == argtypes
    assert "usp_block_select_top_p" in _C.EXPORTS
    assert _C.USP_ATTN_BLOCK_SELECT_TOP_P == 65536 == int(re.search(r"#define USP_ATTN_BLOCK_SELECT_TOP_P (\d+)", txt).group(1))
    L = _C.load()
    assert L.usp_abi_version() == 7 and L.usp_attn_features() & 65536 and L.usp_attn_features() & _C.USP_ATTN_BLOCK_SELECT
    line = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")) if "usp_block_select_top_p" in l]
    assert line and "float top_p" in line[0]


def test_argument_validation_without_launch():
    """Bad arguments are rejected before any launch (safe without a GPU)."""
    from yunchang_amd import _C
    select = _C._select_top_p_entry("usp_block_select_top_p")
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 63) & ~63
    EINVAL, EUNSUP = -1, -2
    ok = dict(B=1, Hq=4, Hkv=2, D=32, nbq=2, nbk=2, row0=0, scale=0.1, causal=1, top_p=0.9, kf=0, kl=1, share=0)

    def sel(q=a, k=a, m=a, strides=(16, 4, 2), **kw):
        p = dict(ok, **kw)
        return select(q, k, p["B"], p["Hq"], p["Hkv"], p["D"], p["nbq"], p["nbk"], p["row0"], p["scale"], p["causal"], p["top_p"],
                      p["kf"], p["kl"], p["share"], m, *strides, None)
    for kw in (dict(q=None), dict(k=None), dict(m=None), dict(B=0), dict(nbq=0), dict(nbk=0), dict(row0=-1), dict(kf=-1), dict(kl=-1),
               dict(kl=0), dict(strides=(16, -4, 2)), dict(scale=float("nan")), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0001),
               dict(top_p=float("nan")), dict(top_p=float("inf"))):
        assert sel(**kw) == EINVAL, kw
    for kw in (dict(D=20), dict(D=136), dict(Hq=3), dict(q=a + 4), dict(nbk=_C.BLOCK_SELECT_MAX_BLOCKS + 1),
               dict(nbk=_C.BLOCK_SELECT_MAX_BLOCKS + 1, share=1)):
        assert sel(**kw) == EUNSUP, kw
    assert _C.load().usp_last_launch_kinds() == 0


# ---- 6. gloo grids in fp64 -----------------------------------------------------------------------------------------------------------------
from dist_util import run_distributed        # noqa: E402

GB, GS, GHQ, GHKV, GD = 1, 512, 4, 2, 16
GSCALE = GD ** -0.5
GSEL = (0.6, 1, 1)


def _grid_inputs():
    g = torch.Generator().manual_seed(43)
    q, k, v, do = (torch.randn(GB, GS, h, GD, generator=g) for h in (GHQ, GHKV, GHKV, GHQ))
    return tuple(t.to(torch.bfloat16) for t in (3 * q, 3 * k, v, do))     # (scores far enough apart to rank in fp32 means)


def _whole_mask(q, k, causal, share):
    """The single-process selection the way the fp64 backend computes it (fp32 means of the padded operands, fp64 from there)."""
    pad = lambda t: torch.nn.functional.pad(t, (0, 32 - GD))
    qbar, kbar = (SR.block_means(pad(t)).to(torch.float32) for t in (q, k))
    return TR.select_from_means(qbar, kbar, GSEL[0], GSCALE, causal, GSEL[1], GSEL[2], share)


def _grid_worker(rank, ws, ud, rd, causal, kind, share):
    import yunchang_amd as Y
    from block_select_top_p_backend import TopPOracleBackend
    from yunchang_amd.kernels import set_block_backend
    from yunchang_amd.ring import ring_flash_attn_func
    be = TopPOracleBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    q, k, v, do = _grid_inputs()
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    loc = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in (q, k, v, do)]
    sel = Y.BlockSelectTopP(*GSEL, share)
    res = {"cases": {}, "masks": {}, "logs": {}}

    def run(fn, name):
        del be.select_log[:], be.masks[:]
        lv = [t.detach().clone().requires_grad_(True) for t in loc[:3]]
        out = fn(*lv)
        out.backward(loc[3])
        res["cases"][name] = [t.detach().float().numpy() for t in (out,) + tuple(x.grad for x in lv)]
        res["masks"][name] = [m.numpy() for m in be.masks]
        res["logs"][name] = list(be.select_log)
    if kind == "ulysses":
        layer = Y.UlyssesAttention(Y.PROCESS_GROUP.ULYSSES_PG)
    else:
        layer = Y.LongContextAttention(ring_impl_type="basic")
    run(lambda a, b, c: layer(a, b, c, causal=causal, block_select=sel), "layer")
    if ud == 1:
        run(lambda a, b, c: ring_flash_attn_func(a, b, c, causal=causal, block_select=sel, group=Y.PROCESS_GROUP.RING_PG), "ring_func")
    if rd > 1:
        refused = []
        for impl in ("zigzag", "strip"):
            try:
                Y.LongContextAttention(ring_impl_type=impl)(*loc[:3], causal=causal, block_select=sel)
                refused.append(False)
            except NotImplementedError as e:
                refused.append("basic ring" in str(e) and "block_select" in str(e))
        res["refused"] = all(refused)
    if ud > 1:        # a KV group split over ulysses ranks: one KV head for two ranks
        try:
            layer(loc[0], loc[1][:, :, :1], loc[2][:, :, :1], causal=causal, block_select=Y.BlockSelectTopP(0.6, share_group=True))
            res["split_refused"] = False
        except NotImplementedError as e:
            res["split_refused"] = "share_group" in str(e)
    return res


@pytest.mark.parametrize("causal,share", [(True, False), (False, True)], ids=["causal", "full-shared"])
@pytest.mark.parametrize("ud,rd,kind", [(1, 2, "hybrid"), (1, 4, "hybrid"), (2, 1, "ulysses"), (2, 2, "hybrid")],
                         ids=["ring2", "ring4", "ulysses2", "hybrid2x2"])
def test_gloo_grids_select_the_rows_of_the_single_process_selection(ud, rd, kind, causal, share):
    """The real layer and ring code with autograd on gloo, pooling and selection by the fp64 backend: every rank selects ONCE per
    call, its rows-only mask is the rows (and heads) of the whole-sequence reference, and out and the gradients are those of the
    block_mask= reference of the gathered sequence.  With share_group (P = 2 ranks, 2 KV heads: whole groups per rank) too."""
    import yunchang_amd as Y
    from yunchang_amd.comm.all_to_all import local_heads
    ws = ud * rd
    res = run_distributed(_grid_worker, ws, ud, rd, causal, kind, share)
    q, k, v, do = _grid_inputs()
    whole = _whole_mask(q, k, causal, share)
    assert 0.2 < float(whole.double().mean()) < 0.9
    truth = BR.ref_all(do, q, k, v, GSCALE, whole, causal)
    truth = (truth[0],) + tuple(truth[2:])
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    n = (GS // rd) // 128
    for rank in range(ws):
        u, r = rank % ud, rank // ud
        want_mask = whole[:, local_heads(GHQ, ud, u), r * n:(r + 1) * n, :]
        want = [ext(t, rank, world_size=ws, rd=rd, ud=ud) for t in truth]
        for name, got in res[rank]["cases"].items():
            masks, log = res[rank]["masks"][name], res[rank]["logs"][name]
            assert len(masks) == 1 and [x[0] for x in log] == ["means", "means", "select_top_p"], (rank, name, log)
            assert log[2][3] == r * n and log[2][2][1] == GS // 128 and log[2][5] == share, (rank, name, log)
            assert torch.equal(torch.from_numpy(masks[0]), want_mask), (rank, name)
            for g, w, what in zip(got, want, ("out", "dq", "dk", "dv")):
                tol = TOL["bfloat16"]["out"] if what == "out" else grad_tol("bfloat16", GHQ // GHKV)
                assert_close(g, w, *tol, f"grid {ud}x{rd} rank {rank} {name} {what}")
        if rd > 1:
            assert res[rank]["refused"]
        if ud > 1:
            assert res[rank]["split_refused"]
