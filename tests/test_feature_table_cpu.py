"""All 64 on/off combinations of (window_size, softcap, alibi_slopes, dropout_p, sinks, cu_doclens) at three levels: the
combination table (kernels/features.py), get_block_backend with a recording backend, and the basic ring's *_func at ring degree
1 on gloo with a recording backend.  No GPU, no library."""
import pytest
import torch

from dist_util import run_distributed

ORDER = ("window_size", "softcap", "alibi_slopes", "dropout_p", "sinks", "cu_doclens")
# The verdicts, written out: key = one bit per argument in ORDER; "ok" = served, "<a>+<b>" = refused with
# "<a> together with <b> is not supported by the HIP attention kernels".
EXPECTED = {
    "000000": "ok",
    "000001": "ok",
    "000010": "ok",
    "000011": "cu_doclens+sinks",
    "000100": "ok",
    "000101": "cu_doclens+dropout_p",
    "000110": "sinks+dropout_p",
    "000111": "cu_doclens+dropout_p",
    "001000": "ok",
    "001001": "cu_doclens+alibi_slopes",
    "001010": "sinks+alibi_slopes",
    "001011": "cu_doclens+alibi_slopes",
    "001100": "dropout_p+alibi_slopes",
    "001101": "cu_doclens+alibi_slopes",
    "001110": "sinks+alibi_slopes",
    "001111": "cu_doclens+alibi_slopes",
    "010000": "ok",
    "010001": "cu_doclens+softcap",
    "010010": "sinks+softcap",
    "010011": "cu_doclens+softcap",
    "010100": "dropout_p+softcap",
    "010101": "cu_doclens+softcap",
    "010110": "sinks+softcap",
    "010111": "cu_doclens+softcap",
    "011000": "alibi_slopes+softcap",
    "011001": "cu_doclens+softcap",
    "011010": "sinks+softcap",
    "011011": "cu_doclens+softcap",
    "011100": "dropout_p+softcap",
    "011101": "cu_doclens+softcap",
    "011110": "sinks+softcap",
    "011111": "cu_doclens+softcap",
    "100000": "ok",
    "100001": "cu_doclens+window_size",
    "100010": "ok",
    "100011": "cu_doclens+window_size",
    "100100": "ok",
    "100101": "cu_doclens+window_size",
    "100110": "sinks+dropout_p",
    "100111": "cu_doclens+window_size",
    "101000": "ok",
    "101001": "cu_doclens+window_size",
    "101010": "sinks+alibi_slopes",
    "101011": "cu_doclens+window_size",
    "101100": "dropout_p+alibi_slopes",
    "101101": "cu_doclens+window_size",
    "101110": "sinks+alibi_slopes",
    "101111": "cu_doclens+window_size",
    "110000": "ok",
    "110001": "cu_doclens+window_size",
    "110010": "sinks+softcap",
    "110011": "cu_doclens+window_size",
    "110100": "dropout_p+softcap",
    "110101": "cu_doclens+window_size",
    "110110": "sinks+softcap",
    "110111": "cu_doclens+window_size",
    "111000": "alibi_slopes+softcap",
    "111001": "cu_doclens+window_size",
    "111010": "sinks+softcap",
    "111011": "cu_doclens+window_size",
    "111100": "dropout_p+softcap",
    "111101": "cu_doclens+window_size",
    "111110": "sinks+softcap",
    "111111": "cu_doclens+window_size",
}
# argument -> the keyword a block launch carries for it
KEYWORD = dict(window_size="window", softcap="softcap", alibi_slopes="alibi", dropout_p="dropout", sinks="sinks", cu_doclens="doc")
B, S, H, D = 1, 16, 2, 64
DOCS = [0, 5, S]


def _on(key):
    return [name for name, bit in zip(ORDER, key) if bit == "1"]


def _values():
    return dict(window_size=(4, 0), softcap=30.0, alibi_slopes=torch.tensor([0.5, 0.25]), dropout_p=0.25,
                sinks=torch.tensor([0.5, -1.0]), cu_doclens=DOCS)


def _refusal(key):
    """The sentence a refused combination must raise, or None."""
    if EXPECTED[key] == "ok":
        return None
    a, b = EXPECTED[key].split("+")
    return f"{a} together with {b} is not supported by the HIP attention kernels"


class Recorder:
    """A block backend that notes the keywords of every flash call and does nothing else."""

    def __init__(self):
        self.calls = []

    def fwd(self, *args, **kw):
        self.calls.append(("fwd", len(args), kw))

    def bwd(self, *args, **kw):
        self.calls.append(("bwd", len(args), kw))

    def fwd_packed(self, *args, **kw):
        self.calls.append(("fwd_packed", len(args), kw))

    def bwd_packed(self, *args, **kw):
        self.calls.append(("bwd_packed", len(args), kw))

    def sink_grad(self, sinks, lse, delta, out=None, accum=False):
        return ("sink_grad", sinks, lse, delta)


def test_the_table_has_every_combination():
    assert sorted(EXPECTED) == [format(i, "06b") for i in range(64)]
    assert sum(v == "ok" for v in EXPECTED.values()) == 11      # nothing; each of the six alone; a window beside each of the four score-level steps


@pytest.mark.parametrize("key", sorted(EXPECTED))
def test_combination_function(key):
    from yunchang_amd.kernels.features import Features
    v = _values()
    f = Features(*(v[name] if name in _on(key) else None for name in ORDER))
    assert f.any() == (key != "000000")
    want = _refusal(key)
    if want is None:
        assert f.check() is f
    else:
        with pytest.raises(NotImplementedError) as e:
            f.check()
        assert str(e.value) == want
    # ... and from flash-attn-style arguments on operands: "off" spelled the way callers spell it
    q = torch.zeros(B, S, H, D, dtype=torch.bfloat16)
    off = dict(window_size=(-1, -1), softcap=0.0, alibi_slopes=None, dropout_p=0.0, sinks=None, cu_doclens=None)
    args = {name: (v[name] if name in _on(key) else off[name]) for name in ORDER}
    if want is None:
        g = Features.of(q, q, True, **args)
        assert [x is not None for x in g] == [bit == "1" for bit in key]
        assert g.softcap in (None, 30.0) and g.dropout in (None, 0.25) and g.window in (None, (4, 0))
    else:
        with pytest.raises(NotImplementedError) as e:
            Features.of(q, q, True, **args)
        assert str(e.value) == want


@pytest.mark.parametrize("key", sorted(k for k in EXPECTED if k[0] == "0"))
def test_block_backend(key):
    """get_block_backend takes no window (a window is a keyword of the launch itself): the 32 combinations without one."""
    from yunchang_amd.kernels import attention as KA
    v, on = _values(), _on(key)
    kw = {KEYWORD[name]: v[name] for name in on}
    if "dropout" in kw:
        kw["dropout"] = (0.25, 77, 3)
    if "doc" in kw:
        kw["doc"] = True
    rec = Recorder()
    prev = KA.set_block_backend(rec)
    try:
        want = _refusal(key)
        if want is not None:
            with pytest.raises(NotImplementedError) as e:
                KA.get_block_backend(**kw)
            assert str(e.value) == want
            return
        be = KA.get_block_backend(**kw)
        if not on:
            assert be is rec                                   # nothing on: the bare backend itself
            return
        launch = {"window": (4, 0)}
        if "dropout" in kw:
            launch["at"] = (8, 4)
        if "doc" in kw:
            launch["doc"] = ("row_lo", "key_hi")
        be.fwd(0, 1, 2, 3, 4, 5, **launch)                     # opens the rows' state
        be.fwd(0, 1, 2, 3, 4, 5, 6, 7, True, **launch)         # merge_in, positional
        be.fwd(0, 1, 2, 3, 4, 5, merge_in=True, **launch)      # merge_in, keyword
        be.bwd(0, 1, 2, **launch)
        carried = {KEYWORD[name] for name in on}
        for i, (what, n_args, seen) in enumerate(rec.calls):
            expect = set(carried) | {"window"} | ({"merge_in"} if i == 2 else set())
            if "sinks" in carried and (what == "bwd" or i in (1, 2)):
                expect.discard("sinks")                        # the sinks ride on the forward launch without merge_in only
            assert set(seen) == expect, (what, i, seen)
            assert seen["window"] == (4, 0)
            if "softcap" in carried:
                assert seen["softcap"] == 30.0
            if "alibi" in carried:
                assert seen["alibi"] is kw["alibi"]
            if "dropout" in carried:
                assert seen["dropout"] == (0.25, 77, 8, 4, 3)  # at=(row0, key0) consumed into the 5-tuple
            if "sinks" in seen:
                assert seen["sinks"] is kw["sinks"]
            if "doc" in carried:
                assert seen["doc"] == ("row_lo", "key_hi")
        if "sinks" in carried:
            assert be.sink_grad("lse", "delta")[:2] == ("sink_grad", kw["sinks"])
        if "doc" in carried:                                   # a launch without its arrays is refused
            for call in (lambda: be.fwd(0, 1, 2), lambda: be.bwd(0, 1, 2), lambda: be.fwd(0, 1, 2, doc=None)):
                with pytest.raises(RuntimeError, match="doc=\\(row_lo, key_hi\\)"):
                    call()
        # the packed calls: softcap passes on, every other feature raises its sentence
        n = len(rec.calls)
        if on == ["softcap"]:
            be.fwd_packed(0, 1, causal=True)
            be.bwd_packed(0, 1, 2)
            assert [c[0] for c in rec.calls[n:]] == ["fwd_packed", "bwd_packed"]
            assert rec.calls[n][2] == {"softcap": 30.0, "causal": True} and rec.calls[n + 1][2] == {"softcap": 30.0}
        else:
            for call in (be.fwd_packed, be.bwd_packed):
                with pytest.raises(NotImplementedError) as e:
                    call(0, 1)
                assert str(e.value) == f"{on[0]} is not supported on packed (variable-length) batches"
            assert len(rec.calls) == n
    finally:
        KA.set_block_backend(prev)


def _ring_worker(rank, ws):
    import yunchang_amd as Y
    from yunchang_amd.kernels import set_block_backend
    rec = Recorder()
    set_block_backend(rec)
    q = torch.zeros(B, S, H, D, dtype=torch.bfloat16)
    v = _values()
    res = {}
    for key in sorted(EXPECTED):
        del rec.calls[:]
        try:
            Y.ring_flash_attn_func(q, q, q, causal=True, **{name: v[name] for name in _on(key)})
        except NotImplementedError as e:
            res[key] = ("refused", str(e), len(rec.calls))
            continue
        res[key] = ("ok", [(what, sorted(k for k, x in kw.items() if x is not None)) for what, _, kw in rec.calls],
                    [kw.get("dropout") for _, _, kw in rec.calls])
    return res


def test_basic_ring_at_degree_one():
    res = run_distributed(_ring_worker, 1)[0]
    assert sorted(res) == sorted(EXPECTED)
    features = set(KEYWORD.values())
    for key, got in sorted(res.items()):
        want = _refusal(key)
        if want is not None:
            assert got == ("refused", want, 0), (key, got)     # ... before any launch
            continue
        assert got[0] == "ok", (key, got)
        calls, dropouts = got[1], got[2]
        assert [what for what, _ in calls] == ["fwd"], (key, calls)       # one block, one launch
        assert set(calls[0][1]) & features == {KEYWORD[name] for name in _on(key)}, (key, calls)
        assert "at" not in calls[0][1]
        if key[3] == "1":                                      # (p, seed, row0, key0, head0): the one block starts at (0, 0), head 0
            p, seed, row0, key0, head0 = dropouts[0]
            assert (p, row0, key0, head0) == (0.25, 0, 0, 0) and 0 <= seed < 1 << 63
