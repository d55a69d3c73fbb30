"""Inputs of the block-selection tests (tests/block_select_ref.py is the reference), CPU tensors from seeded generators:

  white     N(0, 1) noise in q and k: the scores of a row lie close together, so a few rows have a candidate within the fp32
            error of the cut; the CPU test bounds their share on the reference alone.
  planted   the ranking of EVERY row is planted with gaps far above the error: key block J of KV head g carries the one-hot
            centroid e_{(J + 7 g) mod D} on faint noise (needs nb <= D), and row block I of query head h carries
            sum_J w[h, I, J] * (the centroid of J for the KV head of h), the weights a permutation of the grid
            w_max - m / 64 (exact in bf16 and fp16): score[h, I, J] = scale * w[h, I, J] up to the faint noise.  The top weights
            of a row go to the blocks where a selection loop can go wrong -- J = 0, I - 1, I - 2, the last block, J = 63, 64 (the
            list positions 63 / 64 / 65 of the candidate lists) where nb reaches them -- in an order that turns with (h, I); the
            rest follow in a seeded permutation.  Any candidate subset (causal, keep_first, keep_local) keeps the planted order.
  ties      q = 0: every score is 0, the selection is the forced blocks plus the lowest J;
            twins: planted, with key block `b` made a copy of key block `a` < b: the two scores of every row are equal bit for
            bit, and where the cut falls between them the lower J wins."""
import torch

BLOCK = 128
NOISE = 2.0 ** -8


def white(B, S, Hq, Hkv, D, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, S, h, D, generator=g).to(dtype) for h in (Hq, Hkv))


def centroid_dim(J, g, D):
    return (J + 7 * g) % D


def planted_weights(Hq, nb, seed=0):
    """(w (Hq, nb, nb) fp64, order (Hq, nb, nb): order[h, I, m] = the block with the m-th largest weight of row (h, I))."""
    g = torch.Generator().manual_seed(1000 + seed)
    w = torch.empty((Hq, nb, nb), dtype=torch.float64)
    order = torch.empty((Hq, nb, nb), dtype=torch.long)
    w_max = 0.5 + (nb - 1) / 64.0
    for h in range(Hq):
        for I in range(nb):
            special = [j for j in (0, I - 1, I - 2, nb - 1, 63, 64) if 0 <= j < nb]
            special = list(dict.fromkeys(special))
            turn = (h + I) % max(len(special), 1)
            special = special[turn:] + special[:turn]
            rest = [j for j in torch.randperm(nb, generator=g).tolist() if j not in special]
            pri = special + rest
            order[h, I] = torch.tensor(pri)
            w[h, I, torch.tensor(pri)] = w_max - torch.arange(nb, dtype=torch.float64) / 64.0
    return w, order


def planted(B, S, Hq, Hkv, D, dtype=torch.bfloat16, seed=0):
    """(q, k, w, order): see the module docstring."""
    nb = (S + BLOCK - 1) // BLOCK
    assert nb <= D, "one-hot centroids need nb <= D"
    G = Hq // Hkv
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, S, Hq, D, generator=g, dtype=torch.float64) * NOISE
    k = torch.randn(B, S, Hkv, D, generator=g, dtype=torch.float64) * NOISE
    w, order = planted_weights(Hq, nb, seed)
    blk = torch.arange(S) // BLOCK
    for kv in range(Hkv):
        dims = torch.tensor([centroid_dim(J, kv, D) for J in range(nb)])
        k[:, torch.arange(S), kv, dims[blk]] += 1.0
        for h in range(kv * G, (kv + 1) * G):
            add = torch.zeros((nb, D), dtype=torch.float64)
            add[:, dims] = w[h]                                   # row block I: weight of J on J's centroid dim
            q[:, :, h] += add[blk][None]
    return q.to(dtype), k.to(dtype), w, order


def zero_q(B, S, Hq, Hkv, D, dtype=torch.bfloat16, seed=0):
    q, k = white(B, S, Hq, Hkv, D, dtype, seed)
    return torch.zeros_like(q), k


def twins(B, S, Hq, Hkv, D, a, b, dtype=torch.bfloat16, seed=0):
    """planted with key block b a copy of key block a (both whole blocks, a < b)."""
    q, k, w, order = planted(B, S, Hq, Hkv, D, dtype, seed)
    assert a < b and (b + 1) * BLOCK <= S
    k[:, b * BLOCK:(b + 1) * BLOCK] = k[:, a * BLOCK:(a + 1) * BLOCK]
    return q, k


# The cases the CPU test judges on the reference alone and the GPU test runs: (S, Hq, Hkv, D, dtype, seed); nb = 1, 3, 8, 35, 65.
WHITE_CASES = [(64, 4, 2, 32, torch.bfloat16, 1), (300, 4, 2, 64, torch.float16, 2), (1024, 8, 1, 128, torch.bfloat16, 3),
               (4400, 4, 2, 32, torch.bfloat16, 4), (8300, 4, 2, 128, torch.float16, 5)]
PLANTED_CASES = [(64, 4, 2, 32, torch.bfloat16, 1), (300, 4, 2, 32, torch.float16, 2), (1024, 8, 1, 32, torch.bfloat16, 3),
                 (4400, 4, 2, 64, torch.bfloat16, 4), (8300, 4, 2, 128, torch.bfloat16, 5)]


def select_grid(nb):
    """(causal, top_k, keep_first, keep_local) of the selection tests at nb blocks."""
    return [(causal, top_k, kf, kl) for causal in (True, False) for top_k in sorted({0, 1, 3, nb, nb + 5})
            for kf in (0, 2) for kl in (1, 2)]
