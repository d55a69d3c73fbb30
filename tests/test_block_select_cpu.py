"""Top-k block selection (`block_select=`) without a GPU: the fp64 reference (tests/block_select_ref.py) against a brute-force
enumeration, the popcount formula, mutants of the reference that must fail the comparison on the planted inputs, how often the
white-noise cases are ambiguous (judged on the reference alone), the argument logic and refusals of the Python layers, and the
rings and layers on gloo with an fp64 backend (tests/block_select_backend.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import block_mask_ref as BR
import block_select_inputs as X
import block_select_ref as SR
from golden_util import TOL, assert_close, grad_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the reference against a brute-force enumeration ------------------------------------------------------------------------
def brute(q, k, top_k, scale, causal, keep_first, keep_local):
    B, S, Hq, D = q.shape
    Hkv, nb = k.shape[2], (S + 127) // 128
    qn, kn = q.double().numpy(), k.double().numpy()
    out = np.zeros((B, Hq, nb, nb), dtype=bool)
    mean = lambda x, b, blk, h: x[b, blk * 128:min(S, (blk + 1) * 128), h].sum(axis=0) / (min(S, (blk + 1) * 128) - blk * 128)
    for b in range(B):
        for h in range(Hq):
            for I in range(nb):
                vis = [J for J in range(nb) if not causal or J <= I]
                forced = [J for J in vis if J < keep_first or I - keep_local < J <= I]
                rest = [J for J in vis if J not in forced]
                sc = {J: scale * float(mean(qn, b, I, h) @ mean(kn, b, J, h // (Hq // Hkv))) for J in rest}
                best = sorted(rest, key=lambda J: (-sc[J], J))[:max(0, top_k - len(forced))]
                out[b, h, I, forced + best] = True
    return torch.from_numpy(out)


@pytest.mark.parametrize("S,Hq,Hkv,D", [(300, 2, 1, 8), (640, 4, 2, 16), (129, 2, 2, 8)])
def test_reference_matches_brute_force(S, Hq, Hkv, D):
    q, k = X.white(2, S, Hq, Hkv, D, torch.bfloat16, seed=S)
    nb = SR.n_blocks(S)
    for causal, top_k, kf, kl in X.select_grid(nb) + [(False, 2, 0, 0), (False, 1, 1, 0)]:
        got = SR.select_ref(q, k, top_k, 0.37, causal, kf, kl)
        assert torch.equal(got, brute(q, k, top_k, 0.37, causal, kf, kl)), (causal, top_k, kf, kl)


def test_popcount_formula():
    """Every row block selects exactly min(max(top_k, n_forced), n_visible) blocks: top_k = 0 and top_k > nb included."""
    nb = 6
    q, k = X.white(1, nb * 128 - 50, 2, 1, 8, torch.bfloat16, seed=9)
    for causal in (True, False):
        for top_k in range(0, nb + 3):
            for kf in range(0, 4):
                for kl in range(1 if causal else 0, 4):
                    m = SR.select_ref(q, k, top_k, None, causal, kf, kl)
                    want = torch.tensor([SR.popcount(nb, I, top_k, causal, kf, kl) for I in range(nb)])
                    assert torch.equal(m.sum(-1), want.expand(1, 2, nb)), (causal, top_k, kf, kl)
                    if causal:
                        assert not m.triu(1).any() and m.diagonal(dim1=-2, dim2=-1).all()


# ---- 2. the inputs: planted rankings are unambiguous, white noise is rarely ambiguous ----------------------------------------------
@pytest.mark.parametrize("case", X.PLANTED_CASES, ids=lambda c: f"S{c[0]}")
def test_planted_cases_are_unambiguous_and_as_intended(case):
    S, Hq, Hkv, D, dtype, seed = case
    q, k, w, order = X.planted(1, S, Hq, Hkv, D, dtype, seed)
    nb = SR.n_blocks(S)
    prob = SR.Problem(q, k)
    for causal, top_k, kf, kl in X.select_grid(nb):
        j = prob.judge(top_k, causal, kf, kl)
        assert j.ambiguous_rows() == 0.0
        live = ~j.decided
        assert bool((j.gap[live] >= 100 * 2 * j.E[live]).all()), "planted gaps are at least 100 x the tolerance"
        # the intended ranking: the candidates in the order of their planted weights
        visible, forced = SR.candidates(nb, nb, causal, kf, kl)
        cand = (visible & ~forced)
        k_rem = (top_k - forced.sum(-1)).clamp(min=0)
        pos = torch.empty_like(order)
        pos.scatter_(-1, order, torch.arange(nb).expand_as(order))       # rank of J by planted weight
        pos = torch.where(cand[None], pos, torch.full_like(pos, nb))
        rank = pos.argsort(dim=-1).argsort(dim=-1)
        want = forced[None] | (cand[None] & (rank < k_rem[None, :, None]))
        assert torch.equal(j.mask[0], want), (causal, top_k, kf, kl)


@pytest.mark.parametrize("case", X.WHITE_CASES, ids=lambda c: f"S{c[0]}")
def test_white_cases_are_rarely_ambiguous(case):
    """The comparison rule forgives ambiguous candidates; on the cases the GPU test runs at most 5 % of the rows may hold one."""
    S, Hq, Hkv, D, dtype, seed = case
    q, k = X.white(1, S, Hq, Hkv, D, dtype, seed)
    prob = SR.Problem(q, k)
    worst = 0.0
    for causal, top_k, kf, kl in X.select_grid(SR.n_blocks(S)):
        worst = max(worst, prob.judge(top_k, causal, kf, kl).ambiguous_rows())
    print(f"AMBIGUOUS S={S} D={D}: worst share of rows {worst:.4f}, largest eps {float(prob.eps.max()):.3e}")
    assert worst <= 0.05


def test_ties():
    q, k = X.zero_q(1, 1024, 4, 2, 32)
    for causal, top_k, kf, kl in X.select_grid(8):
        m = SR.select_ref(q, k, top_k, None, causal, kf, kl)
        visible, forced = SR.candidates(8, 8, causal, kf, kl)
        cand = visible & ~forced
        low = cand & (cand.cumsum(-1) <= (top_k - forced.sum(-1)).clamp(min=0)[:, None])
        assert torch.equal(m, (forced | low).expand_as(m))
    q, k = X.twins(1, 1024, 4, 2, 32, 2, 5)
    s = SR.Problem(q, k).s
    assert torch.equal(s[..., 2], s[..., 5])
    m = SR.select_ref(q, k, 3, None, False, 0, 1)
    rows = [I for I in range(8) if I not in (2, 5)]                  # (where both twins are candidates)
    assert not bool((m[:, :, rows, 5] & ~m[:, :, rows, 2]).any()) and bool((m[:, :, rows, 2] & ~m[:, :, rows, 5]).any())


# ---- 3. mutants -------------------------------------------------------------------------------------------------------------------
def test_mutants_fail():
    """Each mutant of the reference must fail the comparison the GPU tests make, on the planted inputs."""
    seen = set()
    q, k, _, _ = X.planted(1, 300, 4, 2, 32, torch.bfloat16, 2)
    prob = SR.Problem(q, k)
    ok = SR.select_ref(q, k, 2, None, False, 0, 1)
    assert SR.agrees(ok, prob.judge(2, False, 0, 1))
    assert not SR.agrees(SR.select_ref(q, k, 2, None, False, 0, 1, mutant="last_div128"), prob.judge(2, False, 0, 1))
    seen.add("last_div128")
    q, k, _, _ = X.planted(1, 1024, 4, 2, 32, torch.bfloat16, 3)
    prob = SR.Problem(q, k)
    for name, (top_k, causal, kf, kl) in (("no_diag", (2, True, 0, 1)), ("k_without_forced", (3, True, 0, 1)),
                                          ("wrong_kv_head", (3, False, 0, 1))):
        j = prob.judge(top_k, causal, kf, kl)
        assert SR.agrees(SR.select_ref(q, k, top_k, None, causal, kf, kl), j)
        assert not SR.agrees(SR.select_ref(q, k, top_k, None, causal, kf, kl, mutant=name), j), name
        seen.add(name)
    # the row-block offset of a ring rank: rank 1 of 2 against its rows of the whole selection
    whole = SR.select_ref(q, k, 3, None, True, 0, 1)
    assert torch.equal(SR.select_ref_rows(q, k, 3, 32 ** -0.5, True, 0, 1, 2, 1), whole[:, :, 4:])
    assert not torch.equal(SR.select_ref_rows(q, k, 3, 32 ** -0.5, True, 0, 1, 2, 1, mutant="drop_row_offset"), whole[:, :, 4:])
    seen.add("drop_row_offset")
    # ties: on the twins the comparison is torch.equal (the tied pair is ambiguous by construction, everything else planted)
    q, k = X.twins(1, 1024, 4, 2, 32, 2, 5)
    assert not torch.equal(SR.select_ref(q, k, 3, None, False, 0, 1, mutant="tie_high"), SR.select_ref(q, k, 3, None, False, 0, 1))
    seen.add("tie_high")
    assert seen == set(SR.MUTANTS)


# ---- 4. argument logic ---------------------------------------------------------------------------------------------------------------
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

    def block_select(self, qbar, kbar, top_k, scale, causal, keep_first=0, keep_local=1, row_block0=0):
        self.calls.append(("select", top_k, scale, causal, keep_first, keep_local, row_block0))
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
    """Judged in one place (kernels/features.py: block_select_alone), before any tensor is read."""
    import yunchang_amd as Y
    from yunchang_amd.kernels.attention import hip_attn_forward, hip_attn_func
    from yunchang_amd.kernels.features import block_select_alone
    from yunchang_amd.ring.ring_flash_attn import ring_flash_attn_func
    from yunchang_amd.ring.zigzag_ring_flash_attn import zigzag_ring_flash_attn_func
    q, k, v = _small()
    sel = Y.BlockSelect(2)
    msg = f"block_select together with {name} is not supported by the HIP attention kernels"
    with pytest.raises(NotImplementedError) as e:
        block_select_alone(sel, **kw)
    assert str(e.value) == msg
    for fn in (hip_attn_forward, hip_attn_func, ring_flash_attn_func, zigzag_ring_flash_attn_func):
        with pytest.raises(NotImplementedError) as e:
            fn(q, k, v, causal=True, block_select=sel, **kw)
        assert str(e.value) == msg
    assert recorder.calls == []


def test_other_refusals_and_value_errors(recorder):
    import yunchang_amd as Y
    from yunchang_amd.hybrid.async_attn_layer import AsyncLongContextAttention
    from yunchang_amd.kernels.attention import hip_attn_forward, hip_attn_func, select_blocks
    from yunchang_amd.kernels.features import block_select_alone
    from yunchang_amd.ring import front_end as F
    from yunchang_amd.ring.ring_flash_attn_varlen import ring_flash_attn_varlen_func
    q, k, v = _small()
    sel = Y.BlockSelect(2)
    assert block_select_alone(None) is False and block_select_alone(sel) is True
    assert sel == (2, 0, 1) and Y.BlockSelect(3, 1, 2)._replace(top_k=4) == (4, 1, 2)
    with pytest.raises(AttributeError):
        sel.top_k = 3                                                 # immutable
    with pytest.raises(NotImplementedError, match="return_max_logits together with block_select"):
        hip_attn_func(q, k, v, block_select=sel, return_max_logits=True)
    with pytest.raises(NotImplementedError, match="block_select needs whole q and k of the same length"):
        hip_attn_forward(q, k[:, :128], v[:, :128], block_select=sel)
    with pytest.raises(NotImplementedError, match="same length"):
        select_blocks(q, k[:, :128], 2)
    for bad in ((2, 0, 1), 2, "2"):
        with pytest.raises(ValueError, match="BlockSelect"):
            hip_attn_forward(q, k, v, block_select=bad)
    for bad in (Y.BlockSelect(-1), Y.BlockSelect(2.0), Y.BlockSelect(True), Y.BlockSelect(2, -1), Y.BlockSelect(2, 0, -1),
                Y.BlockSelect(2, 0, 1.5)):
        with pytest.raises(ValueError):
            hip_attn_forward(q, k, v, block_select=bad)
        with pytest.raises(ValueError):
            select_blocks(q, k, bad.top_k, keep_first=bad.keep_first, keep_local=bad.keep_local)
    with pytest.raises(ValueError, match="keep_local >= 1"):
        hip_attn_forward(q, k, v, causal=True, block_select=Y.BlockSelect(2, 0, 0))
    with pytest.raises(ValueError, match="keep_local >= 1"):
        select_blocks(q, k, 2, causal=True, keep_local=0)
    select_blocks(q, k, 2, causal=False, keep_local=0)               # (full attention may keep nothing local)
    with pytest.raises(TypeError):
        select_blocks(q.float(), k.float(), 2)
    with pytest.raises(NotImplementedError, match="variable-length.*ring_flash_attn_func"):
        ring_flash_attn_varlen_func(q[0], k[0], v[0], torch.tensor([0, 256], dtype=torch.int32), 256, block_select=sel)
    with pytest.raises(NotImplementedError, match="block_select.*AsyncLongContextAttention.*LongContextAttention"):
        AsyncLongContextAttention.forward(None, q, k, v, block_select=sel)

    class G4:
        pass
    orig = F.group_info
    F.group_info = lambda dist, group: (4, 1)
    try:
        with pytest.raises(NotImplementedError, match="block_select across ring steps.*zigzag and stripe rings.*basic ring"):
            F._place_block_select(F.DENSE_RING, q, k, F.BlockSelection(sel), True, G4())
        with pytest.raises(NotImplementedError, match="block_select at ring degree 4.*multiple of 128"):
            F._place_block_select(F.BASIC_RING, q[:, :200], k[:, :200], F.BlockSelection(sel), True, G4())
        F._place_block_select(F.BASIC_RING, q, k, F.BlockSelection(sel), True, G4())
    finally:
        F.group_info = orig


def test_none_is_the_call_without_the_keyword_and_the_mask_is_selected_once(recorder):
    import yunchang_amd as Y
    from yunchang_amd.kernels.attention import hip_attn_forward, hip_attn_func
    from yunchang_amd.ring.ring_flash_attn import ring_flash_attn_func
    q, k, v = _small()
    hip_attn_forward(q, k, v, causal=True)
    hip_attn_forward(q, k, v, causal=True, block_select=None)
    assert recorder.calls[0] == recorder.calls[1] and len(recorder.calls) == 2
    del recorder.calls[:]
    hip_attn_forward(q, k, v, causal=True, softmax_scale=0.5, block_select=Y.BlockSelect(3, 1, 2))
    kinds = [c[0] for c in recorder.calls]
    assert kinds == ["means", "means", "select", "fwd"]
    assert recorder.calls[2] == ("select", 3, 0.5, True, 1, 2, 0)
    assert recorder.calls[3][3]["bsp"].dtype == torch.bool
    # autograd: one selection, and the backward runs under the very mask the forward ran under
    import torch.distributed as dist
    own = not dist.is_initialized()                                      # (the ring function asks its group's size)
    if own:
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:29791", rank=0, world_size=1)
    try:
        for fn in (hip_attn_func, lambda *a, **kw: ring_flash_attn_func(*a, group=None, **kw)):
            del recorder.calls[:]
            lq, lk, lv = (t.clone().requires_grad_(True) for t in (q, k, v))
            out = fn(lq, lk, lv, causal=True, block_select=Y.BlockSelect(2))
            out.sum().backward()
            kinds = [c[0] for c in recorder.calls]
            assert kinds == ["means", "means", "select", "fwd", "bwd"], kinds
            assert recorder.calls[4][2]["bsp"] is recorder.calls[3][3]["bsp"]
            assert lq.grad is not None
    finally:
        if own:
            dist.destroy_process_group()


def test_padded_head_dims_select_on_the_padded_operands(recorder):
    """D = 24 runs at 32: the selection pools zero-padded copies (the pad adds 0 to every score) under the scale of D = 24."""
    import yunchang_amd as Y
    from yunchang_amd.kernels.attention import hip_attn_forward
    q = torch.zeros(1, 256, 4, 24, dtype=torch.bfloat16)
    k = torch.zeros(1, 256, 2, 24, dtype=torch.bfloat16)
    hip_attn_forward(q, k, k.clone(), block_select=Y.BlockSelect(1))
    assert recorder.calls[0] == ("means", (1, 256, 4, 32)) and recorder.calls[2][2] == pytest.approx(24 ** -0.5)


def test_rows_only_views():
    """What the basic ring hands the launch of (rank r, step s) from a rank's rows-only mask: mask[..., kr n:(kr + 1) n]."""
    from yunchang_amd.ring.front_end import BlockMask
    from yunchang_amd.ring.ring_flash_attn import _bsp_kw
    P, S_loc = 4, 256
    n, nb = S_loc // 128, P * S_loc // 128
    rows = torch.rand(2, 4, n, nb) < 0.5
    for r in range(P):
        for step in range(P):
            kr = (r - step) % P
            view = _bsp_kw(BlockMask(rows, rows_only=True), r, P, step, S_loc)["bsp"]
            assert tuple(view.shape) == (2, 4, n, n) and view.stride() == rows.stride()
            assert view.data_ptr() == rows.data_ptr() + kr * n * rows.element_size()
    assert _bsp_kw(BlockMask(rows, rows_only=True), 0, 1, 0, S_loc)["bsp"] is rows


# ---- 5. the C ABI surface ---------------------------------------------------------------------------------------------------------
def test_bindings_match_the_header():
    """The struct-free signatures of the two entry points, as tests/test_host_api.py checks the others: every parameter of the
    header's prototype against the ctypes argtypes, the feature bit, the limit."""
    from yunchang_amd import _C
    txt = open(os.path.join(ROOT, "include", "usp_hip.h")).read()
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
             "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    for name in _C.SELECT_EXPORTS:
        proto = re.search(r"\nint " + name + r"\(([^;]*)\);", txt).group(1)
        params = [" ".join(p.split()[:-1]) for p in proto.replace("\n", " ").split(",")]
        bit, _, argtypes = _C._FEATURE_ENTRIES[name]
        assert bit == _C.USP_ATTN_BLOCK_SELECT and [ctype[p] for p in params] == argtypes, name
        assert name in _C.EXPORTS
    assert _C.USP_ATTN_BLOCK_SELECT == 32768 == int(re.search(r"#define USP_ATTN_BLOCK_SELECT (\d+)", txt).group(1))
    assert _C.USP_ATTN_BLOCK_SELECT == 2 * _C.USP_ATTN_MAX_LOGIT
    assert _C.BLOCK_SELECT_MAX_BLOCKS == 8192 == int(re.search(r"#define USP_BLOCK_SELECT_MAX_BLOCKS (\d+)", txt).group(1))
    L = _C.load()
    assert L.usp_abi_version() == 7 and L.usp_attn_features() & _C.USP_ATTN_BLOCK_SELECT


def test_argument_validation_without_launch():
    """Bad arguments are rejected before any launch (safe without a GPU)."""
    from yunchang_amd import _C
    means, select = _C._select_entry("usp_block_means"), _C._select_entry("usp_block_select")
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 63) & ~63
    EINVAL, EUNSUP = -1, -2
    assert means(None, 0, 1, 128, 1, 32, 4096, 32, 32, a, None) == EINVAL
    assert means(a, 0, 1, 128, 1, 32, 4096, 32, 32, None, None) == EINVAL
    assert means(a, 0, 0, 128, 1, 32, 4096, 32, 32, a, None) == EINVAL
    assert means(a, 0, 1, 0, 1, 32, 4096, 32, 32, a, None) == EINVAL
    assert means(a, 7, 1, 128, 1, 32, 4096, 32, 32, a, None) == EINVAL
    assert means(a, 0, 1, 128, 1, 32, 4096, -32, 32, a, None) == EINVAL
    assert means(a, 0, 1, 128, 1, 20, 4096, 32, 32, a, None) == EUNSUP       # D % 8
    assert means(a, 0, 1, 128, 1, 136, 4096, 136, 136, a, None) == EUNSUP    # D > 128
    assert means(a + 2, 0, 1, 128, 1, 32, 4096, 32, 32, a, None) == EUNSUP   # misaligned pointer
    assert means(a, 0, 1, 128, 1, 32, 4096, 36, 32, a, None) == EUNSUP       # misaligned stride
    ok = dict(B=1, Hq=4, Hkv=2, D=32, nbq=2, nbk=2, row0=0, scale=0.1, causal=1, top_k=1, kf=0, kl=1)

    def sel(q=a, k=a, m=a, strides=(16, 4, 2), **kw):
        p = dict(ok, **kw)
        return select(q, k, p["B"], p["Hq"], p["Hkv"], p["D"], p["nbq"], p["nbk"], p["row0"], p["scale"], p["causal"], p["top_k"],
                      p["kf"], p["kl"], m, *strides, None)
    for kw in (dict(q=None), dict(k=None), dict(m=None), dict(B=0), dict(nbq=0), dict(nbk=0), dict(row0=-1), dict(top_k=-1),
               dict(kf=-1), dict(kl=-1), dict(kl=0), dict(strides=(16, -4, 2)), dict(scale=float("nan"))):
        assert sel(**kw) == EINVAL, kw
    for kw in (dict(D=20), dict(D=136), dict(Hq=3), dict(q=a + 4), dict(nbk=_C.BLOCK_SELECT_MAX_BLOCKS + 1)):
        assert sel(**kw) == EUNSUP, kw
    assert _C.load().usp_last_launch_kinds() == 0


# ---- 6. gloo grids in fp64 -----------------------------------------------------------------------------------------------------------
from dist_util import run_distributed        # noqa: E402

GB, GS, GHQ, GHKV, GD = 1, 512, 4, 2, 16
GSCALE = GD ** -0.5
GSEL = (2, 1, 1)


def _grid_inputs():
    g = torch.Generator().manual_seed(41)
    return tuple(torch.randn(GB, GS, h, GD, generator=g).to(torch.bfloat16) for h in (GHQ, GHKV, GHKV, GHQ))


def _whole_mask(q, k, causal):
    """The single-process selection the way the fp64 backend computes it (fp32 means, fp64 scores)."""
    pad = lambda t: torch.nn.functional.pad(t, (0, 32 - GD))
    qbar, kbar = (SR.block_means(pad(t)).to(torch.float32) for t in (q, k))
    return SR.select_from_scores(SR.scores(qbar, kbar, GSCALE), GSEL[0], causal, GSEL[1], GSEL[2])


def _grid_worker(rank, ws, ud, rd, causal, kind):
    import yunchang_amd as Y
    from block_select_backend import SelectOracleBackend
    from yunchang_amd.kernels import set_block_backend
    from yunchang_amd.ring import ring_flash_attn_func
    be = SelectOracleBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    q, k, v, do = _grid_inputs()
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    loc = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in (q, k, v, do)]
    sel = Y.BlockSelect(*GSEL)
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
    return res


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("ud,rd,kind", [(1, 2, "hybrid"), (1, 4, "hybrid"), (2, 1, "ulysses"), (2, 2, "hybrid")],
                         ids=["ring2", "ring4", "ulysses2", "hybrid2x2"])
def test_gloo_grids_select_the_rows_of_the_single_process_selection(ud, rd, kind, causal):
    """The real layer and ring code with autograd on gloo, pooling and selection by the fp64 backend: every rank selects ONCE
    per call, its rows-only mask is the rows (and heads) of the single-process selection, and out and the gradients are those of
    the block_mask= reference of the gathered sequence."""
    import yunchang_amd as Y
    from yunchang_amd.comm.all_to_all import local_heads
    ws = ud * rd
    res = run_distributed(_grid_worker, ws, ud, rd, causal, kind)
    q, k, v, do = _grid_inputs()
    whole = _whole_mask(q, k, causal)
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
            assert len(masks) == 1 and [x[0] for x in log] == ["means", "means", "select"], (rank, name, log)
            assert log[2][3] == r * n and log[2][2][1] == GS // 128, (rank, name, log)
            assert torch.equal(torch.from_numpy(masks[0]), want_mask), (rank, name)
            for g, w, what in zip(got, want, ("out", "dq", "dk", "dv")):
                tol = TOL["bfloat16"]["out"] if what == "out" else grad_tol("bfloat16", GHQ // GHKV)
                assert_close(g, w, *tol, f"grid {ud}x{rd} rank {rank} {name} {what}")
        if rd > 1:
            assert res[rank]["refused"]
