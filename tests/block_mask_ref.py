"""Exact attention in fp64 under a block mask -- global row i sees global key j iff mask[b, h, i // 128, j // 128] and (not causal
or j <= i) -- in the style of tests/interval_ref.py: plain torch on the tensors' device, query rows in chunks of whole row blocks
whose score matrix stays below `chunk_bytes`.  The block mask is expanded to per-row visibility here, from the definition alone:
nothing of the package is imported.

- `mask`: torch.bool (nb, nb), (Hq, nb, nb) or (B, Hq, nb, nb), nb = ceil(S / 128); h is the QUERY head;
- GQA: query head h reads KV head h // (Hq / Hkv);
- rows that see nothing give out = 0, lse = -inf, dq = 0; keys nobody sees get dk = dv = 0;
- `row0`, `key0`: where the launch's row 0 and key 0 lie on the diagonal (a ring block below the diagonal is called with
  causal=False; the diagonal one has row0 == key0).

The mutants of tests/test_block_mask_cpu.py are arguments here, so that the unmutated code path is the one the GPU tests use:
`diag_full` takes the diagonal blocks full instead of causal, `kv_mask` computes dK / dV under another mask than dQ (the
transposed lists built from the untransposed mask)."""
import torch

from attn_ref_torch import CHUNK_BYTES, _heads, _unheads, ref_delta

BLOCK = 128


def n_blocks(S):
    return (S + BLOCK - 1) // BLOCK


def mask4(mask, B, Hq, S):
    """`mask` broadcast to (B, Hq, nb, nb) (a view)."""
    nb = n_blocks(S)
    assert mask.dtype == torch.bool and tuple(mask.shape[-2:]) == (nb, nb), (mask.dtype, tuple(mask.shape), nb)
    if mask.dim() == 2:
        mask = mask[None, None]
    elif mask.dim() == 3:
        mask = mask[None]
    assert mask.shape[1] in (1, Hq) and mask.shape[0] in (1, B), (tuple(mask.shape), B, Hq)
    return mask.expand(B, Hq, nb, nb)


def visible(m4, b, r0, r1, Sk, causal, diag_full=False):
    """(Hq, r1 - r0, Sk) bool: what the rows [r0, r1) of batch entry b see."""
    dev = m4.device
    i = torch.arange(r0, r1, device=dev)
    j = torch.arange(Sk, device=dev)
    vis = m4[b][:, i // BLOCK][:, :, j // BLOCK]
    if causal:
        tri = (j[None, :] // BLOCK <= i[:, None] // BLOCK) if diag_full else (j[None, :] <= i[:, None])
        vis = vis & tri[None]
    return vis


def _row_chunks(Sq, Sk, Hq, chunk_bytes):
    rows = max(BLOCK, (chunk_bytes // (8 * Hq * max(Sk, 1))) // BLOCK * BLOCK)
    for r0 in range(0, Sq, rows):
        yield r0, min(Sq, r0 + rows)


def _scores(qc, kc, vis, scale):
    """qc (Hkv, G, rows, D), kc (Hkv, Sk, D), vis (Hq, rows, Sk) -> S with -inf where hidden (Hkv, G, rows, Sk)."""
    s = torch.matmul(qc, kc.unsqueeze(1).transpose(-1, -2)) * scale
    return s.masked_fill(~vis.reshape(s.shape), float("-inf"))


def ref_fwd(q, k, v, scale, mask, causal=False, diag_full=False, chunk_bytes=CHUNK_BYTES):
    """q (B,S,Hq,D), k / v (B,S,Hkv,D), any float dtype -> (out (B,S,Hq,D), lse (B,Hq,S)) in fp64 on q's device."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    assert Sq == Sk
    m4 = mask4(mask.to(q.device), B, Hq, Sq)
    out = torch.zeros((B, Sq, Hq, D), dtype=torch.float64, device=q.device)
    lse = torch.full((B, Hq, Sq), float("-inf"), dtype=torch.float64, device=q.device)
    for b in range(B):
        kc, vc = (x[b].to(torch.float64).permute(1, 0, 2) for x in (k, v))
        for r0, r1 in _row_chunks(Sq, Sk, Hq, chunk_bytes):
            s = _scores(_heads(q[b], r0, r1, Hkv), kc, visible(m4, b, r0, r1, Sk, causal, diag_full), scale)
            m = s.amax(-1, keepdim=True)
            m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
            p = torch.exp(s - m)
            l = p.sum(-1, keepdim=True)
            row_lse = torch.where(l > 0, m + torch.log(torch.where(l > 0, l, torch.ones_like(l))), torch.full_like(l, float("-inf")))
            lse[b, :, r0:r1] = row_lse[..., 0].reshape(Hq, r1 - r0)
            att = torch.where(l > 0, p / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(p))
            out[b, r0:r1] = _unheads(torch.matmul(att, vc.unsqueeze(1)))
    return out, lse


def ref_bwd(dout, q, k, v, out16, lse, scale, mask, causal=False, diag_full=False, kv_mask=None, chunk_bytes=CHUNK_BYTES):
    """Block backward given the exact lse (B,Hq,S) and the 16-bit out -> (dq, dk, dv, delta), fp64 on q's device:
    P = exp(S - lse), dS = P (dout v^T - delta) scale, delta = rowsum(dout * out16)."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    m4 = mask4(mask.to(q.device), B, Hq, Sq)
    m4kv = m4 if kv_mask is None else mask4(kv_mask.to(q.device), B, Hq, Sq)
    delta = ref_delta(dout, out16)
    lse = lse.to(device=q.device, dtype=torch.float64)
    dq = torch.zeros((B, Sq, Hq, D), dtype=torch.float64, device=q.device)
    dk = torch.zeros((B, Sk, Hkv, D), dtype=torch.float64, device=q.device)
    dv = torch.zeros_like(dk)
    for b in range(B):
        kc, vc = (x[b].to(torch.float64).permute(1, 0, 2) for x in (k, v))
        for r0, r1 in _row_chunks(Sq, Sk, Hq, chunk_bytes):
            rows = r1 - r0
            qc, doc = _heads(q[b], r0, r1, Hkv), _heads(dout[b], r0, r1, Hkv)
            l = lse[b, :, r0:r1].reshape(Hkv, G, rows, 1)
            fin = torch.isfinite(l)
            dl = delta[b, :, r0:r1].reshape(Hkv, G, rows, 1)
            dpv = torch.matmul(doc, vc.unsqueeze(1).transpose(-1, -2)) - dl

            def p_ds(m):
                s = _scores(qc, kc, visible(m, b, r0, r1, Sk, causal, diag_full), scale)
                p = torch.where(fin, torch.exp(s - torch.where(fin, l, torch.zeros_like(l))), torch.zeros_like(s))
                return p, p * dpv * scale
            p, ds = p_ds(m4)
            dq[b, r0:r1] = _unheads(torch.matmul(ds, kc.unsqueeze(1)))
            if kv_mask is not None:
                p, ds = p_ds(m4kv)
            dv[b] += torch.matmul(p.transpose(-1, -2), doc).sum(1).permute(1, 0, 2)
            dk[b] += torch.matmul(ds.transpose(-1, -2), qc).sum(1).permute(1, 0, 2)
    return dq, dk, dv, delta


def ref_all(dout, q, k, v, scale, mask, causal=False, **kw):
    """(out, lse, dq, dk, dv) in fp64, the backward from the forward's out rounded to q's dtype, as the kernels get it."""
    out, lse = ref_fwd(q, k, v, scale, mask, causal, diag_full=kw.get("diag_full", False))
    dq, dk, dv, _ = ref_bwd(dout, q, k, v, out.to(q.dtype), lse, scale, mask, causal, **kw)
    return out, lse, dq, dk, dv


# ---- the lists of usp_block_lists.hip, enumerated (include/usp_hip.h: the block-sparse section) -----------------------------
def enumerate_lists(m4, S, causal):
    """{"fwd": {(b, h, r): [tiles]}, "dq": {(b, h, i): [4 * tile + bits]}, "dkdv": {(b, h, c): [row tiles]}} from a (B, Hq, nb, nb)
    numpy bool array: 64-wide tiles 2c, 2c + 1 of every live block (the second only where the sequence reaches it), ascending,
    the blocks above the diagonal dropped under causal."""
    B, Hq, nb, _ = m4.shape
    nt = (S + 63) // 64
    tiles = lambda c: [t for t in (2 * c, 2 * c + 1) if t < nt]
    live = lambda b, h, r, c: bool(m4[b, h, r, c]) and (not causal or c <= r)
    fwd, dq, dkdv = {}, {}, {}
    for b in range(B):
        for h in range(Hq):
            for r in range(nb):
                fwd[b, h, r] = [t for c in range(nb) if live(b, h, r, c) for t in tiles(c)]
                dkdv[b, h, r] = [t for rr in range(nb) if live(b, h, rr, r) for t in tiles(rr)]
            for i in range((nb + 1) // 2):
                ent = []
                for c in range(nb):
                    bits = (1 if live(b, h, 2 * i, c) else 0) | (2 if 2 * i + 1 < nb and live(b, h, 2 * i + 1, c) else 0)
                    if bits:
                        ent += [4 * t + bits for t in tiles(c)]
                dq[b, h, i] = ent
    return dict(fwd=fwd, dq=dq, dkdv=dkdv)
