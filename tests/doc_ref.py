"""Exact attention in fp64 under a document mask (include/usp_hip.h: usp_flash_fwd_doc / usp_flash_bwd_doc), dense and small: the
truth the document-mask tests hold the block kernels, the basic ring and the layers against.  Written on its own: plain torch on
the tensors' device, one score matrix per call, a boolean mask given explicitly.

    global:  row i sees key j  iff  start(i) <= j <= i,   start(i) = the first position of the document of `cu_doclens` that holds i
    block:   row i sees key j  iff  j >= row_lo[i]  and (causal) j <= i + Sk - Sq          (the launch's own coordinates)

GQA: query head h reads KV head h // (Hq / Hkv); rows without a visible key give lse = -inf, out = 0, dq = 0.

Also the CPU block backend of the orchestration tests with `doc=`: DocOracleBackend.
"""
import numpy as np
import torch

from oracle_backend import OracleBlockBackend


def starts(cu, n):
    """start(i) for i < n: numpy int64."""
    cu = np.asarray(cu, dtype=np.int64)
    return cu[np.searchsorted(cu, np.arange(n), side="right") - 1]


def global_mask(cu_doclens, S, B=1):
    """(B, S, S) bool; `cu_doclens`: one list, or B lists."""
    lists = cu_doclens if isinstance(cu_doclens[0], (list, tuple)) else [cu_doclens] * B
    i = np.arange(S)[:, None]
    j = np.arange(S)[None, :]
    return torch.from_numpy(np.stack([(starts(cu, S)[:, None] <= j) & (j <= i) for cu in lists]))


def block_mask(row_lo, Sq, Sk, causal, B=1):
    """(B, Sq, Sk) bool from a launch's row_lo ((Sq,) or (B, Sq)): j >= row_lo[i], and j <= i + Sk - Sq under causal."""
    rl = torch.as_tensor(np.asarray(row_lo)).to(torch.int64).reshape(-1, Sq).expand(B, Sq)
    i = torch.arange(Sq)[None, :, None]
    j = torch.arange(Sk)[None, None, :]
    m = j >= rl[:, :, None]
    return m & (j <= i + (Sk - Sq)) if causal else m


def mask_of_key_hi(key_hi, Sq, Sk, causal, B=1):
    """The same mask from the transpose: i < key_hi[j]."""
    kh = torch.as_tensor(np.asarray(key_hi)).to(torch.int64).reshape(-1, Sk).expand(B, Sk)
    i = torch.arange(Sq)[None, :, None]
    j = torch.arange(Sk)[None, None, :]
    m = i < kh[:, None, :]
    return m & (j <= i + (Sk - Sq)) if causal else m


def _scores(q, k, scale, mask):
    Hq = q.shape[2]
    k64 = k.to(torch.float64).repeat_interleave(Hq // k.shape[2], dim=2)
    s = torch.einsum("bihd,bjhd->bhij", q.to(torch.float64), k64) * scale
    return s.masked_fill(~mask.to(q.device)[:, None], float("-inf")), k64


def _probs(s, lse):
    fin = torch.isfinite(lse)
    return torch.where(fin[..., None], torch.exp(s - torch.where(fin, lse, torch.zeros_like(lse))[..., None]), torch.zeros_like(s))


def ref_fwd(q, k, v, scale, mask):
    """-> (out (B,Sq,Hq,D), lse (B,Hq,Sq)), fp64 on q's device; mask (B,Sq,Sk) bool."""
    s, _ = _scores(q, k, scale, mask)
    lse = torch.logsumexp(s, dim=-1)
    v64 = v.to(torch.float64).repeat_interleave(q.shape[2] // v.shape[2], dim=2)
    return torch.einsum("bhij,bjhd->bihd", _probs(s, lse), v64), lse


def ref_bwd_from(dout, q, k, v, out, lse, scale, mask):
    """Block backward given the rows' lse and out -> (dq, dk, dv), fp64 (lse / out may be the GLOBAL rows' values)."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    s, k64 = _scores(q, k, scale, mask)
    p = _probs(s, lse.to(torch.float64))
    do64, q64 = dout.to(torch.float64), q.to(torch.float64)
    v64 = v.to(torch.float64).repeat_interleave(G, dim=2)
    delta = (do64 * out.to(torch.float64)).sum(-1).transpose(1, 2)
    ds = p * (torch.einsum("bihd,bjhd->bhij", do64, v64) - delta[..., None]) * scale
    dq = torch.einsum("bhij,bjhd->bihd", ds, k64)
    dk = torch.einsum("bhij,bihd->bjhd", ds, q64).reshape(B, Sk, Hkv, G, D).sum(3)
    dv = torch.einsum("bhij,bihd->bjhd", p, do64).reshape(B, Sk, Hkv, G, D).sum(3)
    return dq, dk, dv


def ref_bwd(dout, q, k, v, scale, mask, out_dtype=None):
    """Forward + backward of the whole problem -> (out, lse, dq, dk, dv), fp64.  `out_dtype`: round `out` to it before delta is
    formed (what a 16-bit kernel's backward reads)."""
    out, lse = ref_fwd(q, k, v, scale, mask)
    o = out if out_dtype is None else out.to(out_dtype)
    return (out, lse) + ref_bwd_from(dout, q, k, v, o, lse, scale, mask)


def needle_edges(cu, S):
    """(row, key) pairs for tests/needle_inputs.py:make(..., edges=...) that make ONE boundary moved by ONE key an O(1) error in
    out AND in every gradient, at one query head per KV head too (where no other head of the group carries a signal):
      - for every boundary s the first rows of the document that starts there (s, s + 1) get a needle on key s - 1, the last key
        of the document in front -- wrongly seen, it takes half the row's mass -- and row s one on its OWN key s: a row whose
        mass sits on one key has dS = 0 whatever it sees, so the wrongly seen needle must share the mass with a rightly seen one
        for dQ and dK to move;
      - for every document [s, e) of three or more positions its last rows (e - 1, e - 2) get needles on its first key s and,
        from four positions on, on s + 1 as well -- wrongly hidden, s takes its share of the mass with it and dS changes on both.
    (A document of one position needs no needle of the second kind: hidden, its row sees nothing.)"""
    out = []
    for s, e in zip(cu[:-1], cu[1:]):
        if s > 0:
            out += [(r, s - 1) for r in (s, s + 1) if r < S] + [(s, s)]
        if e - s >= 3:
            out += [(r, s) for r in (e - 1, e - 2)]
        if e - s >= 4:
            out += [(r, s + 1) for r in (e - 1, e - 2)]
    return out


class DocOracleBackend(OracleBlockBackend):
    """The oracle block backend with `doc=(row_lo, key_hi)` on fwd and bwd: the block is computed here in fp64 under
    block_mask(row_lo) -- the backward under mask_of_key_hi(key_hi) for dK / dV and block_mask(row_lo) for dQ, as the kernels
    read them -- and merged / accumulated the way the kernels' epilogues do.  A launch without the keyword is the wrapped
    oracle's.  Logs every launch in `doc_log`: ("fwd" | "bwd", Sq, Sk, causal, carried the arrays)."""

    def __init__(self):
        super().__init__()
        self.doc_log = []

    def fwd(self, q, k, v, softmax_scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None,
            doc=None, **kw):
        self.doc_log.append(("fwd", q.shape[1], k.shape[1], bool(causal), doc is not None))
        if doc is None:
            return super().fwd(q, k, v, softmax_scale, causal, lse, out, acc, merge_in, final_begin, final_end, **kw)
        B, Sq = q.shape[0], q.shape[1]
        o, l = ref_fwd(q, k, v, softmax_scale, block_mask(doc[0].cpu().numpy(), Sq, k.shape[1], causal, B))
        if merge_in:
            old = lse.to(torch.float64)
            new = torch.logaddexp(old, l)
            fin = torch.isfinite(new)
            w_old = torch.where(fin, torch.exp(old - torch.where(fin, new, torch.zeros_like(new))), torch.zeros_like(new))
            w_blk = torch.where(fin, torch.exp(l - torch.where(fin, new, torch.zeros_like(new))), torch.zeros_like(new))
            o = acc.to(torch.float64) * w_old.transpose(1, 2)[..., None] + o * w_blk.transpose(1, 2)[..., None]
            l = new
        lse.copy_(l)
        fe = Sq if final_end is None else final_end
        for dst, rows in ((out, slice(final_begin, fe)), (acc, slice(0, final_begin)), (acc, slice(fe, Sq))):
            if dst is not None and rows.stop > rows.start:
                dst[:, rows].copy_(o[:, rows])

    def bwd(self, dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale, causal, accum_dq=False, accum_dk=False, accum_dv=False,
            dq16=None, dk16=None, dv16=None, doc=None, **kw):
        self.doc_log.append(("bwd", q.shape[1], k.shape[1], bool(causal), doc is not None))
        if doc is None:
            return super().bwd(dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale, causal, accum_dq, accum_dk, accum_dv,
                               dq16, dk16, dv16, **kw)
        B, Sq, Hq, D = q.shape
        Sk, Hkv = k.shape[1], k.shape[2]
        G = Hq // Hkv
        m_q = block_mask(doc[0].cpu().numpy(), Sq, Sk, causal, B)
        m_k = mask_of_key_hi(doc[1].cpu().numpy(), Sq, Sk, causal, B)
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
             torch.einsum("bhij,bihd->bjhd", ds_k, q64).reshape(B, Sk, Hkv, G, D).sum(3),
             torch.einsum("bhij,bihd->bjhd", p_k, do64).reshape(B, Sk, Hkv, G, D).sum(3))
        for val, d32, d16, accum in zip(g, (dq, dk, dv), (dq16, dk16, dv16), (accum_dq, accum_dk, accum_dv)):
            if accum:
                val = val + d32.to(torch.float64)
            if d16 is not None:
                d16.copy_(val)
            elif d32 is not None:
                d32.copy_(val)
