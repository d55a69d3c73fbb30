"""Block attention mass (`return_block_mass`, block_attention_mass, ring_block_attention_mass) without a GPU: the fp64 reference
pinned against a brute-force pooling of the dense softmax, the mutants its tolerance must reject, the C ABI's argument codes,
every refusal sentence, and the ring / layer schedules on gloo grids over a test-only fp64 backend."""
import ctypes
import os
import re
from collections import Counter

import pytest
import torch

import attn_ref_torch as AR
import block_mass_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(S, Hq, Hkv, D=32, B=1, seed=0, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, S, h, D, generator=g).to(dtype) for h in (Hq, Hkv))


# ---- 1. the reference, pinned ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("S,Hq,Hkv", [(64, 2, 2), (129, 2, 1), (300, 4, 2), (449, 4, 2)])
def test_reference_is_the_pooled_dense_softmax(S, Hq, Hkv, causal):
    q, k = _inputs(S, Hq, Hkv, seed=S)
    scale = 32 ** -0.5
    _, lse = AR.ref_fwd(q, k, k, scale, causal=causal)                       # fp64 (B, Hq, S)
    G = Hq // Hkv
    s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double().repeat_interleave(G, dim=2)) * scale
    if causal:
        s = s.masked_fill(torch.arange(S)[None, :] > torch.arange(S)[:, None], float("-inf"))
    P = torch.softmax(s, dim=-1)
    assert torch.allclose(torch.logsumexp(s, -1), lse, rtol=0, atol=1e-12)
    nb = (S + 127) // 128
    brute = torch.zeros(1, Hq, nb, nb, dtype=torch.float64)
    for I in range(nb):
        for J in range(nb):
            blk = P[:, :, 128 * I:128 * (I + 1), 128 * J:128 * (J + 1)]
            brute[:, :, I, J] = blk.sum(dim=(-1, -2)) / blk.shape[-2]
    ref = MR.mass_ref(q, k, lse, scale, causal)
    assert ref.shape == (1, Hq, nb, nb)
    assert torch.allclose(ref, brute, rtol=1e-12, atol=1e-300)
    assert torch.allclose(ref.sum(-1), torch.ones(1, Hq, nb, dtype=torch.float64), rtol=1e-12, atol=0)
    if causal:
        assert float(ref.triu(1).abs().max()) == 0.0
    # a row with lse = -inf contributes 0: the other rows of its block still average over rows(I)
    l2 = lse.clone()
    l2[:, :, 0] = float("-inf")
    r2 = MR.mass_ref(q, k, l2, scale, causal)
    rows0 = min(128, S)
    assert torch.allclose(r2[:, :, 0].sum(-1), torch.full((1, Hq), (rows0 - 1) / rows0, dtype=torch.float64), rtol=1e-12, atol=0)


def test_ring_slices_assemble_to_the_whole_map():
    q, k = _inputs(512, 4, 2, seed=5)
    scale = 32 ** -0.5
    for causal in (True, False):
        lse = MR.dense_lse(q, k, scale, causal)
        whole = MR.mass_ref(q, k, lse, scale, causal)
        for P in (2, 4):
            assert torch.equal(MR.ring_assembled(q, k, lse, scale, causal, P), whole) or \
                torch.allclose(MR.ring_assembled(q, k, lse, scale, causal, P), whole, rtol=1e-13, atol=0)


# ---- 2. mutants ------------------------------------------------------------------------------------------------------------
MUTANTS = ["lost_tile", "tail_unmasked", "diag_off", "kv_head", "lse_head", "div128", "transposed", "ring_diag"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_miss_the_bound(mutant):
    """Each wrong kernel, in fp64, misses the derived bound by 2 x and more on white noise at S = 449, Hq 4 / Hkv 2 (causal;
    the ring mutant at S = 512, whole blocks per rank)."""
    scale = 32 ** -0.5
    if mutant == "ring_diag":
        q, k = _inputs(512, 4, 2, seed=11)
        lse = MR.dense_lse(q, k, scale, True)
        ref = MR.mass_ref(q, k, lse, scale, True)
        bad = MR.ring_assembled(q, k, lse, scale, True, 2, mutant="ring_diag")
    else:
        q, k = _inputs(449, 4, 2, seed=11)
        lse = MR.dense_lse(q, k, scale, True)
        ref = MR.mass_ref(q, k, lse, scale, True)
        bad = MR.mass_ref(q, k, lse, scale, True, mutant=mutant)
    d = MR.exponent_error(q, k, lse, scale)
    assert MR.misses(ref, ref, d) == 0.0
    miss = MR.misses(bad, ref, d)
    print(f"mutant {mutant}: {miss:.3g} x the bound")
    assert miss >= 2.0, (mutant, miss)


def test_bound_is_a_few_ulp():
    """The bound on white noise at D = 128 stays near 1e-5 relative: it separates the mutants because it is tight."""
    q, k = _inputs(300, 2, 1, D=128, seed=3)
    scale = 128 ** -0.5
    lse = MR.dense_lse(q, k, scale, True)
    d = MR.exponent_error(q, k, lse, scale)
    assert float(d.max()) < 2e-4
    assert MR.SUM_DEPTH == 74 and MR.E_SUM == 74 * 2.0 ** -24 and 1e-7 < MR.E_EXP < 1e-6


# ---- 3. the C ABI ----------------------------------------------------------------------------------------------------------
def test_binding_matches_the_header():
    from yunchang_amd import _C
    txt = open(os.path.join(ROOT, "include", "usp_hip.h")).read()
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
             "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    proto = re.search(r"\nint usp_block_attn_mass\(([^;]*)\);", txt).group(1)
    params = [p.split() for p in proto.replace("\n", " ").split(",")]
    assert [p[-1] for p in params] == ["q", "k", "lse", "dtype", "B", "Sq", "Sk", "Hq", "Hkv", "D", "q_stride_b", "q_stride_s",
                                       "q_stride_h", "k_stride_b", "k_stride_s", "k_stride_h", "lse_stride_b", "lse_stride_h",
                                       "scale", "causal", "diag", "out", "out_stride_b", "out_stride_h", "out_stride_row", "stream"]
    bit, _, argtypes = _C._FEATURE_ENTRIES["usp_block_attn_mass"]
    assert bit == _C.USP_ATTN_BLOCK_MASS and [ctype[" ".join(p[:-1])] for p in params] == argtypes
    assert "usp_block_attn_mass" in _C.EXPORTS and _C.MASS_EXPORTS == ("usp_block_attn_mass",)
    assert _C.USP_ATTN_BLOCK_MASS == 131072 == int(re.search(r"#define USP_ATTN_BLOCK_MASS (\d+)", txt).group(1))
    L = _C.load()
    assert L.usp_abi_version() == 7 and L.usp_attn_features() & 131072
    assert L.usp_attn_features() & _C.USP_ATTN_BLOCK_SELECT_TOP_P and L.usp_attn_features() & _C.USP_ATTN_BLOCK_SELECT
    assert "usp_block_mass.hip" in open(os.path.join(ROOT, "long-context-attention_amd", "csrc", "Makefile")).read()


def test_argument_validation_without_launch():
    """Bad arguments are rejected before any launch (safe without a GPU)."""
    from yunchang_amd import _C
    mass = _C._mass_entry("usp_block_attn_mass")
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 63) & ~63
    EINVAL, EUNSUP = -1, -2
    ok = dict(dtype=0, B=1, Sq=256, Sk=256, Hq=4, Hkv=2, D=32, scale=0.1, causal=1, diag=0)

    def call(q=a, k=a, lse=a, out=a, qs=(32768, 128, 32), ks=(16384, 64, 32), ls=(1024, 256), os_=(16, 4, 2), **kw):
        p = dict(ok, **kw)
        return mass(q, k, lse, p["dtype"], p["B"], p["Sq"], p["Sk"], p["Hq"], p["Hkv"], p["D"], *qs, *ks, *ls, p["scale"],
                    p["causal"], p["diag"], out, *os_, None)
    for kw in (dict(q=None), dict(k=None), dict(lse=None), dict(out=None), dict(B=0), dict(Sq=0), dict(Sk=-1), dict(Hq=0), dict(Hkv=0),
               dict(D=0), dict(dtype=2), dict(qs=(32768, -128, 32)), dict(ks=(-1, 64, 32)), dict(ls=(1024, -256)), dict(os_=(16, 4, -2)),
               dict(scale=float("nan"))):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(D=20), dict(D=256), dict(D=96), dict(Hq=3), dict(q=a + 4), dict(k=a + 8), dict(qs=(32768, 132, 32)),
               dict(ks=(16384, 64, 36)), dict(lse=a + 2), dict(out=a + 1), dict(diag=1 << 30), dict(ks=(16384, 1 << 24, 32))):
        assert call(**kw) == EUNSUP, kw
    assert _C.load().usp_last_launch_kinds() == 0


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------
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

    def block_mass(self, q, k, lse, scale, causal, diag=0, out=None):
        self.calls.append(("mass", tuple(q.shape), tuple(k.shape), scale, causal, diag))
        nbq, nbk = (q.shape[1] + 127) // 128, (k.shape[1] + 127) // 128
        return torch.zeros(q.shape[0], q.shape[2], nbq, nbk) if out is None else out.zero_()


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


def _refused():
    import yunchang_amd as Y
    return [("window_size", dict(window_size=(64, 0))), ("softcap", dict(softcap=30.0)), ("alibi_slopes", dict(alibi_slopes=torch.ones(4))),
            ("dropout_p", dict(dropout_p=0.1)), ("sinks", dict(sinks=torch.zeros(4))), ("cu_doclens", dict(cu_doclens=[0, 128, 256])),
            ("bidirectional", dict(bidirectional=[(0, 8)])), ("block_mask", dict(block_mask=torch.ones(2, 2, dtype=torch.bool))),
            ("block_select", dict(block_select=Y.BlockSelect(2))), ("return_max_logits", dict(return_max_logits=True))]


@pytest.mark.parametrize("idx", range(10))
def test_refusal_table(recorder, idx):
    """`return_block_mass together with ...`: one sentence everywhere, before any tensor is read or anything launched."""
    import yunchang_amd as Y
    from yunchang_amd.kernels.attention import hip_attn_forward, hip_attn_func
    from yunchang_amd.kernels.features import return_block_mass_alone
    from yunchang_amd.ring.ring_flash_attn import ring_flash_attn_func, ring_flash_attn_kvpacked_func, ring_flash_attn_qkvpacked_func
    from yunchang_amd.ring.stripe_flash_attn import stripe_flash_attn_func
    from yunchang_amd.ring.zigzag_ring_flash_attn import zigzag_ring_flash_attn_func
    name, kw = _refused()[idx]
    q, k, v = _small()
    msg = f"return_block_mass together with {name} is not supported by the HIP attention kernels"
    with pytest.raises(NotImplementedError) as e:
        return_block_mass_alone(True, **kw)
    assert str(e.value) == msg
    calls = [lambda: fn(q, k, v, causal=True, return_block_mass=True, **kw)
             for fn in (hip_attn_forward, hip_attn_func, ring_flash_attn_func, zigzag_ring_flash_attn_func, stripe_flash_attn_func)]
    calls += [lambda: ring_flash_attn_kvpacked_func(q, torch.stack([q, q], 2), causal=True, return_block_mass=True, **kw),
              lambda: ring_flash_attn_qkvpacked_func(torch.stack([q, q, q], 2), causal=True, return_block_mass=True, **kw),
              lambda: Y.UlyssesAttention.forward(None, q, k, v, causal=True, return_block_mass=True, **kw),
              lambda: Y.LongContextAttention.forward(None, q, k, v, causal=True, return_block_mass=True, **kw),
              lambda: Y.LongContextAttentionQKVPacked.forward(None, torch.stack([q, q, q], 2), causal=True, return_block_mass=True, **kw)]
    for call in calls:
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == msg
    assert recorder.calls == []
    assert return_block_mass_alone(False, **kw) is False and return_block_mass_alone(None, **kw) is False


def test_other_refusals(recorder):
    import yunchang_amd as Y
    from yunchang_amd.hybrid.async_attn_layer import AsyncLongContextAttention
    from yunchang_amd.kernels import block_attention_mass as k_mass, block_mask_recall as k_recall
    from yunchang_amd.kernels.attention import block_attention_mass, block_mask_recall, hip_attn_forward, hip_attn_func
    from yunchang_amd.kernels.features import return_block_mass_alone
    from yunchang_amd.ring import front_end as F, ring_block_attention_mass
    from yunchang_amd.ring.ring_flash_attn_varlen import (ring_flash_attn_varlen_func, ring_flash_attn_varlen_kvpacked_func,
                                                          ring_flash_attn_varlen_qkvpacked_func)
    from yunchang_amd.ring.zigzag_ring_flash_attn_varlen import zigzag_ring_flash_attn_varlen_func
    q, k, v = _small()
    lse = torch.zeros(1, 4, 256)
    assert Y.block_attention_mass is block_attention_mass is k_mass and Y.block_mask_recall is block_mask_recall is k_recall
    assert Y.ring_block_attention_mass is ring_block_attention_mass is F.ring_block_attention_mass
    assert return_block_mass_alone(True) is True and return_block_mass_alone(True, softcap=0.0, dropout_p=0.0, window_size=(-1, -1)) is True
    # q and k of different lengths
    for call in (lambda: hip_attn_forward(q, k[:, :128], v[:, :128], return_block_mass=True),
                 lambda: hip_attn_func(q, k[:, :128], v[:, :128], return_block_mass=True)):
        with pytest.raises(NotImplementedError, match="return_block_mass needs whole q and k of the same length"):
            call()
    with pytest.raises(NotImplementedError, match="block_attention_mass needs whole q and k of the same length"):
        block_attention_mass(q, k[:, :128], lse)
    with pytest.raises(ValueError, match="lse"):
        block_attention_mass(q, k, lse[:, :, :100])
    with pytest.raises(TypeError):
        block_attention_mass(q.float(), k.float(), lse)
    # packed batches and the varlen rings
    cu = torch.tensor([0, 256], dtype=torch.int32)
    for call in (lambda: ring_flash_attn_varlen_func(q[0], k[0], v[0], cu, 256, return_block_mass=True),
                 lambda: zigzag_ring_flash_attn_varlen_func(q[0], k[0], v[0], cu, 256, return_block_mass=True),
                 lambda: ring_flash_attn_varlen_kvpacked_func(q[0], torch.stack([q[0], q[0]], 1), cu, 256, return_block_mass=True),
                 lambda: ring_flash_attn_varlen_qkvpacked_func(torch.stack([q[0]] * 3, 1), cu, 256, return_block_mass=True)):
        with pytest.raises(NotImplementedError, match="return_block_mass is not supported by the variable-length \\(packed\\) rings.*"
                                                      "ring_flash_attn_func"):
            call()
    with pytest.raises(NotImplementedError, match="return_block_mass.*AsyncLongContextAttention.*use LongContextAttention"):
        AsyncLongContextAttention.forward(None, q, k, v, return_block_mass=True)

    class G4:
        pass
    orig = F.group_info
    F.group_info = lambda dist, group: (4, 1)
    try:
        run = lambda probs: (_ for _ in ()).throw(AssertionError("the forward ran"))
        with pytest.raises(NotImplementedError, match="return_block_mass across ring steps.*zigzag and stripe rings.*basic ring"):
            F.block_mass_call(F.DENSE_RING, run, q, k, None, True, G4(), False)
        with pytest.raises(NotImplementedError, match="return_block_mass at ring degree 4.*multiple of 128"):
            F.block_mass_call(F.BASIC_RING, run, q[:, :200], k[:, :200], None, True, G4(), False)
        with pytest.raises(NotImplementedError, match="return_block_mass needs whole q and k of the same length"):
            F.block_mass_call(F.BASIC_RING, run, q, k[:, :128], None, True, G4(), False)
        with pytest.raises(NotImplementedError, match="ring_block_attention_mass at ring degree 4.*multiple of 128"):
            ring_block_attention_mass(q[:, :200], k[:, :200], lse[:, :, :200], group=G4())
    finally:
        F.group_info = orig
    assert recorder.calls == []


def test_keyword_runs_the_plain_call_and_then_the_map(recorder):
    """hip_attn_forward / hip_attn_func: the forward launch of the call without the keyword, then ONE block_mass on the padded
    operands with the scale of the unpadded head dim; block_mask_recall is plain torch."""
    from yunchang_amd.kernels.attention import block_mask_recall, hip_attn_forward, hip_attn_func
    q, k, v = _small()
    out, lse, mass = hip_attn_forward(q, k, v, causal=True, return_block_mass=True)
    assert [c[0] for c in recorder.calls] == ["fwd", "mass"] and recorder.calls[0][3] == {"window": None}
    assert recorder.calls[1][1:] == ((1, 256, 4, 32), (1, 256, 2, 32), 32 ** -0.5, True, 0)
    assert mass.shape == (1, 4, 2, 2) and mass.dtype == torch.float32 and not mass.requires_grad
    del recorder.calls[:]
    q40, k40 = q[..., :24].clone().requires_grad_(True), k[..., :24].clone()
    res = hip_attn_func(q40, k40, k40, causal=False, return_block_mass=True)
    assert len(res) == 2 and res[0].shape == q40.shape and res[1].shape == (1, 4, 2, 2) and not res[1].requires_grad
    assert [c[0] for c in recorder.calls] == ["fwd", "mass"]
    assert recorder.calls[1][1:] == ((1, 256, 4, 32), (1, 256, 2, 32), 24 ** -0.5, False, 0)
    res = hip_attn_func(q, k, v, return_attn_probs=True, return_block_mass=True)
    assert len(res) == 4 and res[2] is None and res[1].shape == (1, 4, 256) and res[3].shape == (1, 4, 2, 2)
    m = torch.rand(1, 4, 2, 3)
    mask = torch.tensor([[True, False, True], [False, False, True]])
    assert torch.allclose(block_mask_recall(m, mask), torch.stack([m[..., 0, 0] + m[..., 0, 2], m[..., 1, 2]], -1))
    assert torch.allclose(block_mask_recall(m, torch.ones(2, 3, dtype=torch.bool)), m.sum(-1))


# ---- 5. schedules on gloo grids, fp64 backend -------------------------------------------------------------------------------
from dist_util import run_distributed        # noqa: E402

GB, GS, GHQ, GHKV, GD = 1, 512, 4, 2, 32
GSCALE = GD ** -0.5


def _grid_inputs():
    g = torch.Generator().manual_seed(47)
    q, k, v = (torch.randn(GB, GS, h, GD, generator=g) for h in (GHQ, GHKV, GHKV))
    return tuple(t.to(torch.bfloat16) for t in (q, k, v))


def _grid_worker(rank, ws, ud, rd, causal, kind):
    import torch.distributed as dist
    import yunchang_amd as Y
    from block_mass_backend import MassOracleBackend
    from yunchang_amd.kernels import set_block_backend
    from yunchang_amd.ring import ring_block_attention_mass, ring_flash_attn_func
    be = MassOracleBackend()
    set_block_backend(be)
    Y.set_seq_parallel_pg(ud, rd, rank, ws)
    q, k, v = _grid_inputs()
    ext = Y.EXTRACT_FUNC_DICT["basic"]
    loc = [ext(t, rank, world_size=ws, rd=rd, ud=ud).detach().clone() for t in (q, k, v)]
    sends = []
    real = dist.batch_isend_irecv

    def counted(ops):
        sends.extend(tuple(op.tensor.shape) for op in ops if op.op is dist.isend)
        return real(ops)
    dist.batch_isend_irecv = counted
    res = {}
    layer = Y.UlyssesAttention(Y.PROCESS_GROUP.ULYSSES_PG) if kind == "ulysses" else Y.LongContextAttention(ring_impl_type="basic")
    plain = layer(*loc, causal=causal)
    res["sends_plain"] = list(sends)
    del sends[:], be.mass_log[:]
    out, mass = layer(*loc, causal=causal, return_block_mass=True)
    res["sends_mass"] = list(sends)
    res["same_out"] = bool(torch.equal(out, plain))
    res["layer"] = mass.numpy()
    res["layer_log"] = list(be.mass_log)
    res["no_grad"] = not mass.requires_grad and mass.dtype == torch.float32
    if ud == 1:
        o2, lse, _ = ring_flash_attn_func(*loc, causal=causal, return_attn_probs=True, group=Y.PROCESS_GROUP.RING_PG)
        del sends[:], be.mass_log[:]
        res["alone"] = ring_block_attention_mass(loc[0], loc[1], lse, causal=causal, group=Y.PROCESS_GROUP.RING_PG).numpy()
        res["alone_sends"] = list(sends)
        res["alone_log"] = list(be.mass_log)
        del sends[:]
        o3, m3 = ring_flash_attn_func(*loc, causal=causal, return_block_mass=True, group=Y.PROCESS_GROUP.RING_PG)
        res["func_same"] = bool(torch.equal(o3, o2)) and bool(torch.equal(m3, torch.from_numpy(res["alone"])))
    if rd > 1:
        refused = []
        for impl in ("zigzag", "strip"):
            try:
                Y.LongContextAttention(ring_impl_type=impl)(*loc, causal=causal, return_block_mass=True)
                refused.append(False)
            except NotImplementedError as e:
                refused.append("basic ring" in str(e) and "return_block_mass across ring steps" in str(e))
        res["refused"] = all(refused)
    dist.batch_isend_irecv = real
    return res


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("ud,rd,kind", [(1, 2, "hybrid"), (1, 4, "hybrid"), (2, 1, "ulysses"), (2, 2, "hybrid")],
                         ids=["ring2", "ring4", "ulysses2", "hybrid2x2"])
def test_gloo_grids_assemble_the_whole_map(ud, rd, kind, causal):
    """The real ring and layer code on gloo over the fp64 backend: every rank's share is its heads and its ring shard's row blocks
    of the whole-sequence reference; K makes rd - 1 hops and nothing else travels for the map (V makes none); under causal the
    steps above the diagonal launch nothing; every step writes its own column slice with diag = s * S_local."""
    from yunchang_amd.comm.all_to_all import local_heads
    ws = ud * rd
    res = run_distributed(_grid_worker, ws, ud, rd, causal, kind)
    q, k, v = _grid_inputs()
    ref = MR.mass_ref(q, k, MR.dense_lse(q, k, GSCALE, causal), GSCALE, causal)
    Sl = GS // rd
    n, nb = Sl // 128, GS // 128
    hq_l, hkv_l = GHQ // ud, max(1, GHKV // ud)
    for rank in range(ws):
        u, r = rank % ud, rank // ud
        got = res[rank]
        want = ref[:, local_heads(GHQ, ud, u), r * n:(r + 1) * n, :]
        steps = [s for s in range(rd) if not causal or s <= r]
        for name in ("layer",) + (("alone",) if ud == 1 else ()):
            m = torch.from_numpy(got[name]).double()
            assert m.shape == (GB, hq_l, n, nb), (rank, name, m.shape)
            assert torch.allclose(m, want, rtol=1e-5, atol=1e-30), (rank, name, float((m - want).abs().max()))
            log = got[name + "_log"]
            assert len(log) == len(steps), (rank, name, log)
            for s, entry in zip(steps, log):
                qs, ks, c, diag, oshape, ostride, ooff = entry
                assert qs == (GB, Sl, hq_l, GD) and ks == (GB, Sl, hkv_l, GD) and c == causal and diag == s * Sl, (rank, name, entry)
                if rd > 1:
                    assert oshape == (GB, hq_l, n, n) and ostride[2] == nb and ooff == ((r - s) % rd) * n, (rank, name, entry)
            if causal:                                              # the slices of the steps that launched nothing are zero
                assert float(m[..., (r + 1) * n:].abs().max()) == 0.0 if r + 1 < rd else True
        assert got["same_out"] and got["no_grad"]
        extra = Counter(got["sends_mass"]) - Counter(got["sends_plain"])
        assert extra == (Counter({(GB, Sl, hkv_l, GD): rd - 1}) if rd > 1 else Counter()), (rank, extra)
        assert not (Counter(got["sends_plain"]) - Counter(got["sends_mass"]))
        if ud == 1:
            assert got["alone_sends"] == [(GB, Sl, GHKV, GD)] * (rd - 1), (rank, got["alone_sends"])
            assert got["func_same"]
        if rd > 1:
            assert got["refused"]
