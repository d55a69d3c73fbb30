"""Reference of the gathered-key forward (include/usp_hip.h: USP_ATTN_KEY_INDEX): the boolean mask from the definition, and fp64
softmax attention under it on the operands' device.  Imports nothing from the package."""
import torch


def mask(Sq, Sk, key_index, left=None):
    """(B, Hq, Sq, Sk) bool from a (B, Hq, n) integer list: row i (d_i = i + Sk - Sq) sees key j iff j <= d_i and (d_i - j <= left, when
    a band is given, or j is listed).  An entry outside [0, Sk) is absent."""
    dev = key_index.device
    B, Hq, _ = key_index.shape
    d = torch.arange(Sq, device=dev)[:, None] + (Sk - Sq)
    j = torch.arange(Sk, device=dev)[None, :]
    idx = key_index.long()
    ok = (idx >= 0) & (idx < Sk)
    listed = torch.zeros(B, Hq, Sk + 1, dtype=torch.bool, device=dev)
    listed.scatter_(2, torch.where(ok, idx, torch.full_like(idx, Sk)), True)
    seen = listed[:, :, None, :Sk].expand(B, Hq, Sq, Sk)
    if left is not None:
        seen = seen | (d - j <= left)
    return seen & (j <= d)


def attention(q, k, v, scale, m):
    """(out (B, Sq, Hq, D), lse (B, Hq, Sq)) in fp64 under the mask m; a row that sees nothing: out = 0, lse = -inf."""
    G = q.shape[2] // k.shape[2]
    kd, vd = (t.double().repeat_interleave(G, dim=2) for t in (k, v))
    s = torch.einsum("bihd,bjhd->bhij", q.double(), kd) * scale
    s = s.masked_fill(~m, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.masked_fill(lse == float("-inf"), 0.0)[..., None])
    return torch.einsum("bhij,bjhd->bihd", p, vd), lse
