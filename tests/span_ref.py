"""Exact attention in fp64 under bidirectional spans (include/usp_hip.h: usp_flash_fwd_span / usp_flash_bwd_span), dense and small:
the truth the span tests hold the block kernels, the basic ring and the layers against.  Written on its own: plain torch on the
tensors' device, one score matrix per call, a boolean mask given explicitly and built from the GLOBAL definition alone:

    global:  row i sees key j  iff  start(i) <= j < hi(i)
             start(i) = the first position of the document of `cu_doclens` that holds i (0 without cu_doclens)
             hi(i)    = the end e of the span [s, e) that holds i, i + 1 where no span does
    block:   row i sees key j  iff  row_lo[i] <= j < row_hi[i]   ( = key_lo[j] <= i < key_hi[j] )     (the launch's own coordinates)

GQA: query head h reads KV head h // (Hq / Hkv); rows without a visible key give lse = -inf, out = 0, dq = 0.

Also the CPU block backend of the orchestration tests with `span=`: SpanOracleBackend (tests/doc_ref.py's with one more keyword).
"""
import numpy as np
import torch

from doc_ref import DocOracleBackend


def global_mask(S, cu_doclens=None, spans=(), B=1):
    """(B, S, S) bool from the definition, pair by pair; `cu_doclens` / `spans`: one list or B lists each (None: one document)."""
    def per_batch(x, is_one):
        return [x] * B if is_one else list(x)
    cus = per_batch(cu_doclens if cu_doclens is not None else [0, S],
                    cu_doclens is None or not isinstance(cu_doclens[0], (list, tuple)))
    one_list = len(spans) == 0 or (len(spans[0]) == 2 and all(isinstance(x, (int, np.integer)) for x in spans[0]))
    sps = per_batch(spans, one_list)
    out = np.zeros((B, S, S), dtype=bool)
    for b in range(B):
        start = np.zeros(S, dtype=np.int64)
        for s, e in zip(cus[b][:-1], cus[b][1:]):
            start[s:e] = s
        hi = np.arange(S, dtype=np.int64) + 1
        for s, e in sps[b]:
            hi[s:e] = e
        j = np.arange(S)[None, :]
        out[b] = (start[:, None] <= j) & (j < hi[:, None])
    return torch.from_numpy(out)


def block_mask(row_lo, row_hi, Sq, Sk, B=1):
    """(B, Sq, Sk) bool from a launch's row arrays ((Sq,) or (B, Sq)): row_lo[i] <= j < row_hi[i]."""
    lo = torch.as_tensor(np.asarray(row_lo)).to(torch.int64).reshape(-1, Sq).expand(B, Sq)
    hi = torch.as_tensor(np.asarray(row_hi)).to(torch.int64).reshape(-1, Sq).expand(B, Sq)
    j = torch.arange(Sk)[None, None, :]
    return (j >= lo[:, :, None]) & (j < hi[:, :, None])


def mask_of_keys(key_lo, key_hi, Sq, Sk, B=1):
    """The same mask from the transpose: key_lo[j] <= i < key_hi[j]."""
    lo = torch.as_tensor(np.asarray(key_lo)).to(torch.int64).reshape(-1, Sk).expand(B, Sk)
    hi = torch.as_tensor(np.asarray(key_hi)).to(torch.int64).reshape(-1, Sk).expand(B, Sk)
    i = torch.arange(Sq)[None, :, None]
    return (i >= lo[:, None, :]) & (i < hi[:, None, :])


def _scores(q, k, scale, mask):
    G = q.shape[2] // k.shape[2]
    k64 = k.to(torch.float64).repeat_interleave(G, dim=2)
    s = torch.einsum("bihd,bjhd->bhij", q.to(torch.float64), k64) * scale
    return s.masked_fill(~mask.to(q.device)[:, None], float("-inf")), k64


def _probs(s, lse):
    fin = torch.isfinite(lse)
    safe = torch.where(fin, lse, torch.zeros_like(lse))
    return torch.where(fin[..., None], torch.exp(s - safe[..., None]), torch.zeros_like(s))


def ref_fwd(q, k, v, scale, mask):
    """-> (out (B,Sq,Hq,D), lse (B,Hq,Sq)), fp64 on q's device; mask (B,Sq,Sk) bool."""
    s, _ = _scores(q, k, scale, mask)
    lse = torch.logsumexp(s, dim=-1)
    v64 = v.to(torch.float64).repeat_interleave(q.shape[2] // v.shape[2], dim=2)
    return torch.einsum("bhij,bjhd->bihd", _probs(s, lse), v64), lse


def ref_bwd_from(dout, q, k, v, out, lse, scale, mask_q, mask_k=None):
    """Block backward given the rows' lse and out -> (dq, dk, dv), fp64.  `mask_q` masks the dQ side, `mask_k` (default: the
    same) the dK / dV side -- the kernels read the row arrays for one and the key arrays for the other."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    do64, q64 = dout.to(torch.float64), q.to(torch.float64)
    v64 = v.to(torch.float64).repeat_interleave(G, dim=2)
    delta = (do64 * out.to(torch.float64)).sum(-1).transpose(1, 2)
    dp = torch.einsum("bihd,bjhd->bhij", do64, v64) - delta[..., None]

    def side(mask):
        s, k64 = _scores(q, k, scale, mask)
        p = _probs(s, lse.to(torch.float64))
        return p, p * dp * scale, k64
    _, ds_q, k64 = side(mask_q)
    p_k, ds_k, _ = side(mask_q if mask_k is None else mask_k)
    dq = torch.einsum("bhij,bjhd->bihd", ds_q, k64)
    dk = torch.einsum("bhij,bihd->bjhd", ds_k, q64).reshape(B, Sk, Hkv, G, D).sum(3)
    dv = torch.einsum("bhij,bihd->bjhd", p_k, do64).reshape(B, Sk, Hkv, G, D).sum(3)
    return dq, dk, dv


def ref_bwd(dout, q, k, v, scale, mask, out_dtype=None):
    """Forward + backward of the whole problem -> (out, lse, dq, dk, dv), fp64.  `out_dtype`: round `out` to it before delta is
    formed (what a 16-bit kernel's backward reads)."""
    out, lse = ref_fwd(q, k, v, scale, mask)
    o = out if out_dtype is None else out.to(out_dtype)
    return (out, lse) + ref_bwd_from(dout, q, k, v, o, lse, scale, mask)


def needle_edges(spans, S, cu=None):
    """(row, key) pairs for tests/needle_inputs.py:make(..., edges=...) that make ONE span end or start moved by ONE key or row an
    O(1) error in out AND in every gradient (tests/doc_ref.py: needle_edges explains why a wrongly seen or hidden needle must
    share the row's mass with a rightly seen one for dS to move).  For every span [s, e) of two or more positions:
      - its first rows (s, s + 1 if inside) get needles on the LAST key inside, e - 1, and the first key behind, e (if e < S and
        still in the row's document): e - 1 wrongly hidden (the end one key early) or e wrongly seen (one key late) moves half
        the row's mass; each of these rows also keeps one on its own key, rightly seen either way;
      - the row just in front of the span, s - 1 (if any, and in the same document), gets needles on its own key and on key s:
        the span's start one row early lets it see the whole span, key s first;
      - the last row inside, e - 1, gets needles on key e (wrongly seen when the end comes one key late) and on key s (rightly
        seen), and the row just behind, e (if < S and in the same document), on its own key and on key e - 1, both rightly seen:
        its row must not change whichever way the end moves."""
    start = np.zeros(S + 1, dtype=np.int64)
    for a, b in zip((cu or [0, S])[:-1], (cu or [0, S])[1:]):
        start[a:b] = a
    out = []
    for s, e in spans:
        if e - s < 2:
            continue
        rows = [r for r in (s, s + 1) if r < e - 1] or [s]
        for r in rows:
            out += [(r, r), (r, e - 1)]
            if e < S and start[e] == start[r]:
                out.append((r, e))
        if e < S and start[e] == start[e - 1]:
            out += [(e - 1, e), (e - 1, s)]
        if s > 0 and start[s - 1] == start[s]:
            out += [(s - 1, s - 1), (s - 1, s)]
        if e < S and start[e] <= e - 1:
            out += [(e, e), (e, e - 1)]
    return sorted(set(out))


class SpanOracleBackend(DocOracleBackend):
    """tests/doc_ref.py's oracle block backend with `span=(row_lo, row_hi, key_lo, key_hi)` on fwd and bwd: the block is computed
    here in fp64 under block_mask(row_lo, row_hi) -- the backward's dK / dV under mask_of_keys(key_lo, key_hi), as the kernels
    read them -- and merged / accumulated the way the kernels' epilogues do.  A launch without the keyword is the wrapped
    backend's.  Logs every span launch in `span_log`: ("fwd" | "bwd", Sq, Sk, causal)."""

    def __init__(self):
        super().__init__()
        self.span_log = []

    def fwd(self, q, k, v, softmax_scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None,
            span=None, **kw):
        if span is None:
            return super().fwd(q, k, v, softmax_scale, causal, lse, out, acc, merge_in, final_begin, final_end, **kw)
        assert not causal and all(x is None for x in kw.values()), "a span launch is never causal and carries no other option"
        self.span_log.append(("fwd", q.shape[1], k.shape[1], bool(causal)))
        B, Sq = q.shape[0], q.shape[1]
        o, l = ref_fwd(q, k, v, softmax_scale, block_mask(span[0].cpu().numpy(), span[1].cpu().numpy(), Sq, k.shape[1], B))
        if merge_in:
            old = lse.to(torch.float64)
            new = torch.logaddexp(old, l)
            fin = torch.isfinite(new)
            safe = torch.where(fin, new, torch.zeros_like(new))
            w_old = torch.where(fin, torch.exp(old - safe), torch.zeros_like(new))
            w_blk = torch.where(fin, torch.exp(l - safe), torch.zeros_like(new))
            o = acc.to(torch.float64) * w_old.transpose(1, 2)[..., None] + o * w_blk.transpose(1, 2)[..., None]
            l = new
        lse.copy_(l)
        fe = Sq if final_end is None else final_end
        for dst, rows in ((out, slice(final_begin, fe)), (acc, slice(0, final_begin)), (acc, slice(fe, Sq))):
            if dst is not None and rows.stop > rows.start:
                dst[:, rows].copy_(o[:, rows])

    def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale, causal, accum_dq=False, accum_dk=False, accum_dv=False,
            dq16=None, dk16=None, dv16=None, span=None, **kw):
        if span is None:
            return super().bwd(dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale, causal, accum_dq, accum_dk, accum_dv,
                               dq16, dk16, dv16, **kw)
        assert not causal and all(x is None for x in kw.values()), "a span launch is never causal and carries no other option"
        self.span_log.append(("bwd", q.shape[1], k.shape[1], bool(causal)))
        B, Sq, Hq, D = q.shape
        Sk = k.shape[1]
        a = [t.cpu().numpy() for t in span]
        m_q, m_k = block_mask(a[0], a[1], Sq, Sk, B), mask_of_keys(a[2], a[3], Sq, Sk, B)
        # (delta is given: rebuild an `out` stand-in is not needed -- form dP - delta directly)
        G = Hq // k.shape[2]
        do64, q64 = dout.to(torch.float64), q.to(torch.float64)
        v64 = v.to(torch.float64).repeat_interleave(G, dim=2)
        dp = torch.einsum("bihd,bjhd->bhij", do64, v64) - delta.to(torch.float64)[..., None]

        def side(mask):
            s, k64 = _scores(q, k, softmax_scale, mask)
            p = _probs(s, lse.to(torch.float64))
            return p, p * dp * softmax_scale, k64
        _, ds_q, k64 = side(m_q)
        p_k, ds_k, _ = side(m_k)
        g = (torch.einsum("bhij,bjhd->bihd", ds_q, k64),
             torch.einsum("bhij,bihd->bjhd", ds_k, q64).reshape(B, Sk, k.shape[2], G, D).sum(3),
             torch.einsum("bhij,bihd->bjhd", p_k, do64).reshape(B, Sk, k.shape[2], G, D).sum(3))
        for val, d32, d16, accum in zip(g, (dq, dk, dv), (dq16, dk16, dv16), (accum_dq, accum_dk, accum_dv)):
            if accum:
                val = val + d32.to(torch.float64)
            if d16 is not None:
                d16.copy_(val)
            elif d32 is not None:
                d32.copy_(val)
