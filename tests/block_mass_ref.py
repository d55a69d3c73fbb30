"""The reference of the block attention mass (include/usp_hip.h: usp_block_attn_mass), dense and small, in fp64:

    mass[b, h, I, J] = (1 / rows(I)) * sum_{i in I, i < Sq} sum_{j in J, j visible to i} exp(scale * q[b,i,h] . k[b,j,h // G] - lse[b,h,i])

computed from the 16-bit operands as given AND THE VERY fp32 lse HANDED TO THE KERNEL, so the lse's own error is no part of the
comparison.  Every key j < Sk is visible, under causal only j <= i + diag; a row with lse = -inf contributes 0; rows(I) is the
number of rows block I has.

The tolerance is derived, not chosen.  All terms are non-negative, so the bound is relative:

    |got - ref| <= ref * (expm1(d) + E_EXP + E_SUM + 2^-23) + 128 * 2^-126

  d      the error of the exponent, in natural units, per (batch, head):
           - the score: the MFMA-chain bound of tests/max_logit_ref.py, 2 scale Dp 2^-24 max_pairs sum_d |q_d k_d| (products of
             16-bit operands are exact in fp32; what remains is the fp32 accumulation over the Dp terms, any order);
           - the exponent expression as the kernel writes it, x = fma(s, c, nl) with c = fl(fl(scale) * fl(log2 e)) and
             nl = -fl(lse * fl(log2 e)), u = 2^-24: the score path is rounded four times (scale to fp32 at the C ABI, log2 e to
             fp32, their product, the fma), the lse path three times (log2 e, the product, the fma), each a relative error of at
             most u on a term of size log2(e) |s| or log2(e) |lse|; back in natural units (times ln 2) that is
             4 u |s| + 3 u |lse| + O(u^2) <= K_ROUND u (max |s| + max |lse|), K_ROUND = 5 covering the second-order terms;
         a relative error of the probability of expm1(d);
  E_EXP  twice the measured relative error of the device's exp2 (v_exp_f32) over EVERY fp32 argument in [-126, 0]:
         tools/exp2_error.hip on one MI355X printed 8.4839e-08 (0.712 ulp of 2^-23) at x = -1.93753684 -- taken once, over the
         whole range a probability <= 1 can come from, and doubled;
  E_SUM  the depth of the documented summation order times 2^-24: 64 terms of a lane in sequence, the row's two halves (1), the
         butterfly over the 32 rows (5), the four waves (3), the division (1) = 74;
  2^-23  the fp32 result itself (and slack for the reference's own fp64 arithmetic);
  128 * 2^-126  a probability below 2^-126 leaves v_exp_f32 as 0: at most 2^-126 per (row, key), 128 keys per row of a block, the
         mean over the rows no larger."""
import torch

BLOCK = 128
E_EXP = 2 * 8.4839e-08
SUM_DEPTH = 64 + 1 + 5 + 3 + 1
E_SUM = SUM_DEPTH * 2.0 ** -24
K_ROUND = 5
FLUSH = 128 * 2.0 ** -126


def kernel_head_dim(D):
    return next(d for d in (32, 64, 128) if D <= d)


def _blocks(n):
    return (n + BLOCK - 1) // BLOCK


def probs(q, k, lse, scale, causal=False, diag=0, mutant=None):
    """(B, Hq, Sq, Sk) fp64: exp(scale q.k - lse) where visible, 0 elsewhere.  `mutant`: a wrong kernel (tests only)."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    q64, k64 = q.to(torch.float64), k.to(torch.float64)
    if mutant == "kv_head":                        # the KV head h in place of h // G
        kx = k64[:, :, [h % Hkv for h in range(Hq)]]
    else:
        kx = k64.repeat_interleave(G, dim=2)
    s = torch.einsum("bihd,bjhd->bhij", q64, kx) * scale
    l = lse.to(torch.float64)
    if mutant == "lse_head":                       # the lse of the neighbouring head
        l = l.roll(1, dims=1)
    p = torch.exp(s - l[..., None])
    p = torch.where(torch.isinf(l)[..., None] & (l[..., None] < 0), torch.zeros_like(p), p)
    i = torch.arange(Sq, device=q.device)[:, None]
    j = torch.arange(Sk, device=q.device)[None, :]
    d = diag + (1 if mutant == "diag_off" else 0)  # the diagonal one key off
    vis = (j <= i + d) if causal else torch.ones(Sq, Sk, dtype=torch.bool, device=q.device)
    if mutant == "tail_unmasked" and causal:       # the tail tile left unmasked: every key of the row's last 64-key tile
        vis = j < ((i + d) // 64 + 1) * 64
    if mutant == "lost_tile":                      # a lost 64-key tile (the second of the sequence)
        vis = vis & ~((j >= 64) & (j < 128))
    return torch.where(vis, p, torch.zeros_like(p))


def mass_ref(q, k, lse, scale, causal=False, diag=0, mutant=None):
    """(B, Hq, nbq, nbk) fp64."""
    p = probs(q, k, lse, scale, causal, diag, mutant)
    B, Hq, Sq, Sk = p.shape
    nbq, nbk = _blocks(Sq), _blocks(Sk)
    p = torch.nn.functional.pad(p, (0, nbk * BLOCK - Sk, 0, nbq * BLOCK - Sq))
    m = p.view(B, Hq, nbq, BLOCK, nbk, BLOCK).sum(dim=(3, 5))
    rows = torch.tensor([min(BLOCK, Sq - I * BLOCK) for I in range(nbq)], dtype=torch.float64, device=p.device)
    if mutant == "div128":                         # division by 128 in a ragged block
        rows = torch.full_like(rows, BLOCK)
    m = m / rows[None, None, :, None]
    if mutant == "transposed":
        m = m.transpose(-1, -2).contiguous()
    return m


def ring_assembled(q, k, lse, scale, causal, P, mutant=None):
    """The whole map assembled from the slice launches of a basic ring of degree P (rank r, step s: the keys of rank r - s with
    diag = s * S_local), the way ring_block_attention_mass writes them.  `mutant` "ring_diag": diag one block off."""
    B, S, Hq, _ = q.shape
    Sl = S // P
    n = Sl // BLOCK
    out = torch.zeros(B, Hq, P * n, P * n, dtype=torch.float64, device=q.device)
    for r in range(P):
        for s in range(P):
            if causal and s > r:
                continue
            kr = (r - s) % P
            diag = s * Sl - (BLOCK if mutant == "ring_diag" else 0)
            out[:, :, r * n:(r + 1) * n, kr * n:(kr + 1) * n] = mass_ref(
                q[:, r * Sl:(r + 1) * Sl], k[:, kr * Sl:(kr + 1) * Sl], lse[:, :, r * Sl:(r + 1) * Sl], scale, causal, diag)
    return out


def exponent_error(q, k, lse, scale):
    """d of the bound, (B, Hq) fp64."""
    G = q.shape[2] // k.shape[2]
    q64 = q.to(torch.float64)
    k64 = k.to(torch.float64).repeat_interleave(G, dim=2)
    Dp = kernel_head_dim(q.shape[3])
    pairs = torch.einsum("bihd,bjhd->bhij", q64.abs(), k64.abs()).amax(dim=(-1, -2))
    smax = (torch.einsum("bihd,bjhd->bhij", q64, k64) * scale).abs().amax(dim=(-1, -2))
    l = lse.to(torch.float64)
    lmax = torch.where(torch.isinf(l), torch.zeros_like(l), l.abs()).amax(dim=-1)
    return 2.0 * abs(scale) * Dp * 2.0 ** -24 * pairs + K_ROUND * 2.0 ** -24 * (smax + lmax)


def tolerance(ref, d):
    """The bound, elementwise on ref (B, Hq, nbq, nbk) with d (B, Hq)."""
    rel = torch.expm1(d)[..., None, None] + E_EXP + E_SUM + 2.0 ** -23
    return ref * rel + FLUSH


def check(got, ref, d, what=""):
    """Asserts the bound; prints the largest error as a share of it first.  Returns that share."""
    got = got.detach().to(ref.device).to(torch.float64)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} against {tuple(ref.shape)}"
    assert not torch.isnan(got).any(), f"{what}: NaN"
    share = float(((got - ref).abs() / tolerance(ref, d)).max())
    print(f"MASSERR {what} {share:.3f} of the bound (largest |err| {float((got - ref).abs().max()):.3e}, d {float(d.max()):.2e})")
    assert share <= 1.0, f"{what}: {share:.3f} x the bound"
    return share


def misses(mutant, ref, d):
    """By how many times the bound a wrong map misses it."""
    return float(((mutant - ref).abs() / tolerance(ref, d)).max())


def dense_lse(q, k, scale, causal=False):
    """The fp32 lse (B, Hq, Sq) of the plain softmax, computed in fp64 and rounded once: what a forward hands over."""
    G = q.shape[2] // k.shape[2]
    s = torch.einsum("bihd,bjhd->bhij", q.to(torch.float64), k.to(torch.float64).repeat_interleave(G, dim=2)) * scale
    if causal:
        Sq, Sk = s.shape[-2:]
        s = s.masked_fill(torch.arange(Sk, device=s.device)[None, :] > torch.arange(Sq, device=s.device)[:, None] + (Sk - Sq), float("-inf"))
    return torch.logsumexp(s, dim=-1).to(torch.float32)
