"""The reference of the top-k block selection (`block_select=`, kernels/attention.py: select_blocks; include/usp_hip.h:
usp_block_means, usp_block_select), in fp64, written from the definition alone -- nothing of the package is imported:

    qbar[b, I, h] = mean of the rows of block I of q (a ragged last block: over the rows it has); kbar likewise
    score[b, h, I, J] = scale * qbar[b, I, h] . kbar[b, J, h // G]
    visible: every J, under causal J <= I;  forced: J < keep_first and I - keep_local < J <= I, of the visible ones
    selected = forced + the best max(0, top_k - n_forced) of the other visible ones by (score descending, J ascending)

I is the GLOBAL row block: `row_block0` + the local index (a ring rank selects its own rows against all key blocks).

The mutants of tests/test_block_select_cpu.py are arguments here (`mutant=`), so the unmutated path is the one the GPU tests use.

The tolerance is derived, not chosen.  The kernels work in fp32 (u = 2^-24) in a documented order:
  * a mean: the 16-bit inputs are exact in fp32; a block's rows are added in 8 runs of 16 rows, ascending, and the runs
    ascending; every addition rounds once, so |sum32 - sum| <= u * (sum of the |partial sums| the kernel forms) to first order
    (the running error bound of recursive summation), and the division rounds once more:  e_mean = (u * P + u * |sum|) / count,
    P taken from the same partial sums in fp64;
  * a score: one chain of fused multiply-adds over ascending d, one rounding a step: u * sum_d |partial dot_d|; the operands'
    own errors enter as sum_d (e_q |kbar| + e_k |qbar| + e_q e_k); the product by the fp32 scale rounds twice: 2 u |score|.
`score_eps` is the sum of these, times 1 + 2^-10 for the second-order terms.  (Zero padding of the head dim adds exact zeros.)

The comparison rule (`compare`): with cut = the midpoint of the last selected and the first rejected fp64 score of a row, a
candidate is AMBIGUOUS when |score - cut| <= eps(I, J) + max_J' eps(I, J').  (Why the row maximum is added: every unambiguous
selected block then has an fp32 score above cut + E and every unambiguous rejected one below cut - E, E the row maximum, while a
reference-selected ambiguous one stays above cut - E and a reference-rejected one below cut + E; so the k best fp32 scores hold
every unambiguous selected block and no unambiguous rejected one, whatever the ambiguous ones do.)  The kernel's row must hold
every unambiguous selected block, no unambiguous rejected one, exactly the forced blocks among the non-candidates, and as many
blocks as the reference's row."""
import torch

BLOCK = 128
U = 2.0 ** -24
RUNS, RUN_ROWS = 8, 16
MUTANTS = ("last_div128", "no_diag", "tie_high", "k_without_forced", "wrong_kv_head", "drop_row_offset")


def n_blocks(S):
    return (S + BLOCK - 1) // BLOCK


def block_means(x, mutant=None, with_error=False):
    """x (B, S, H, D) -> fp64 (B, nb, H, D) means; with_error: also the bound e_mean of the fp32 kernel's mean, same shape."""
    B, S, H, D = x.shape
    nb = n_blocks(S)
    x64 = x.to(torch.float64)
    pad = nb * BLOCK - S
    if pad:
        x64 = torch.cat([x64, torch.zeros((B, pad, H, D), dtype=torch.float64, device=x.device)], dim=1)
    count = torch.full((nb,), float(BLOCK), dtype=torch.float64, device=x.device)
    if pad and mutant != "last_div128":
        count[-1] = BLOCK - pad
    runs = x64.reshape(B, nb, RUNS, RUN_ROWS, H, D)
    total = runs.sum(dim=(2, 3))
    mean = total / count[None, :, None, None]
    if not with_error:
        return mean
    within = runs.cumsum(dim=3)                                   # the partial sums of a run (the first is no addition)
    run_sums = within[:, :, :, -1]
    across = run_sums.cumsum(dim=2)
    P = within[:, :, :, 1:].abs().sum(dim=(2, 3)) + across[:, :, 1:].abs().sum(dim=2)
    return mean, (U * P + U * total.abs()) / count[None, :, None, None]


def kv_head(h, Hq, Hkv, mutant=None):
    return h % Hkv if mutant == "wrong_kv_head" else h // (Hq // Hkv)


def scores(qbar, kbar, scale, mutant=None):
    """fp64 (B, Hq, nbq, nbk) from means (B, nbq, Hq, D), (B, nbk, Hkv, D)."""
    Hq, Hkv = qbar.shape[2], kbar.shape[2]
    idx = torch.tensor([kv_head(h, Hq, Hkv, mutant) for h in range(Hq)], device=qbar.device)
    return torch.einsum("bihd,bjhd->bhij", qbar.to(torch.float64), kbar.to(torch.float64)[:, :, idx]) * scale


def score_eps(qbar, eq, kbar, ek, scale):
    """The bound of |score32 - score64| (module docstring), fp64 (B, Hq, nbq, nbk)."""
    Hq, Hkv = qbar.shape[2], kbar.shape[2]
    idx = torch.tensor([kv_head(h, Hq, Hkv) for h in range(Hq)], device=qbar.device)
    kb, ekb = kbar[:, :, idx], ek[:, :, idx]
    prod = torch.einsum("bihd,bjhd->bhijd", qbar, kb)
    chain = prod.cumsum(dim=-1).abs().sum(dim=-1)
    s = prod.sum(dim=-1)
    operands = (torch.einsum("bihd,bjhd->bhij", eq, kb.abs()) + torch.einsum("bihd,bjhd->bhij", qbar.abs(), ekb)
                + torch.einsum("bihd,bjhd->bhij", eq, ekb))
    return (abs(scale) * (U * chain + operands) + 2 * U * (s * scale).abs()) * (1 + 2.0 ** -10)


def candidates(nbq, nbk, causal, keep_first, keep_local, row_block0=0, mutant=None, device="cpu"):
    """(visible, forced) bool (nbq, nbk)."""
    if mutant == "drop_row_offset":
        row_block0 = 0
    I = torch.arange(nbq, device=device)[:, None] + row_block0
    J = torch.arange(nbk, device=device)[None, :]
    visible = (J <= I) if causal else torch.ones((nbq, nbk), dtype=torch.bool, device=device)
    local = (J > I - keep_local) & (J <= I)
    if mutant == "no_diag":
        local = local & (J != I)
    forced = ((J < keep_first) | local) & visible
    return visible, forced


def select_from_scores(s, top_k, causal=False, keep_first=0, keep_local=1, row_block0=0, mutant=None):
    """bool (B, Hq, nbq, nbk) from fp64 scores of that shape: a stable sort by (-score, J)."""
    nbq, nbk = s.shape[-2:]
    visible, forced = candidates(nbq, nbk, causal, keep_first, keep_local, row_block0, mutant, s.device)
    cand = visible & ~forced
    n_forced = forced.sum(dim=-1)
    k_rem = torch.full_like(n_forced, top_k) if mutant == "k_without_forced" else (top_k - n_forced).clamp(min=0)
    key = torch.where(cand, -s, torch.full_like(s, float("inf")))
    if mutant == "tie_high":
        order = key.flip(-1).sort(dim=-1, stable=True).indices
        order = nbk - 1 - order
    else:
        order = key.sort(dim=-1, stable=True).indices
    rank = torch.empty_like(order)
    rank.scatter_(-1, order, torch.arange(nbk, device=s.device).expand_as(order))
    return forced | (cand & (rank < k_rem[:, None]))


def select_ref(q, k, top_k, scale=None, causal=False, keep_first=0, keep_local=1, mutant=None):
    """The whole-sequence reference mask, bool (B, Hq, nb, nb)."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    s = scores(block_means(q, mutant), block_means(k, mutant), scale, mutant)
    return select_from_scores(s, top_k, causal, keep_first, keep_local, 0, mutant)


def select_ref_rows(q, k, top_k, scale, causal, keep_first, keep_local, P, r, mutant=None):
    """What ring rank r of P selects: its rows of the whole sequence against all key blocks, bool (B, Hq, n, nb)."""
    n = n_blocks(q.shape[1]) // P
    qbar = block_means(q[:, r * n * BLOCK:(r + 1) * n * BLOCK], mutant)
    s = scores(qbar, block_means(k, mutant), scale, mutant)
    return select_from_scores(s, top_k, causal, keep_first, keep_local, r * n, mutant)


def popcount(nb, I, top_k, causal, keep_first, keep_local):
    """min(max(top_k, n_forced), n_visible) of row block I, in closed form."""
    nv = min(I + 1, nb) if causal else nb
    forced = {j for j in range(nv) if j < keep_first or I - keep_local < j <= I}
    return min(max(top_k, len(forced)), nv)


class Problem:
    """The fp64 means, scores and error bounds of one (q, k, scale): what every selection of it is judged from."""

    def __init__(self, q, k, scale=None):
        self.scale = q.shape[-1] ** -0.5 if scale is None else scale
        self.qbar, self.eq = block_means(q, with_error=True)
        self.kbar, self.ek = block_means(k, with_error=True)
        self.s = scores(self.qbar, self.kbar, self.scale)
        self.eps = score_eps(self.qbar, self.eq, self.kbar, self.ek, self.scale)

    def judge(self, top_k, causal=False, keep_first=0, keep_local=1):
        return Judged(self, top_k, causal, keep_first, keep_local)


class Judged:
    """The reference selection of a problem with what `compare` needs: mask, ambiguous (both (B, Hq, nb, nb) bool), and per row
    `gap` (last selected - first rejected score; +inf where no score decides anything) and `E` (the largest eps of the row)."""

    def __init__(self, problem, top_k, causal=False, keep_first=0, keep_local=1):
        self.s, self.eps = problem.s, problem.eps
        nb = self.s.shape[-1]
        visible, forced = candidates(nb, nb, causal, keep_first, keep_local, device=self.s.device)
        self.cand = (visible & ~forced).expand_as(self.s)
        self.mask = select_from_scores(self.s, top_k, causal, keep_first, keep_local)
        sel, rej = self.mask & self.cand, ~self.mask & self.cand
        inf = torch.full_like(self.s, float("inf"))
        last = torch.where(sel, self.s, inf).amin(dim=-1)                  # +inf: nothing selected by score
        first = torch.where(rej, self.s, -inf).amax(dim=-1)                # -inf: nothing rejected
        self.decided = ~(torch.isfinite(last) & torch.isfinite(first))    # rows where no score decides anything
        self.gap = torch.where(self.decided, inf[..., 0], last - first)
        cut = torch.where(self.decided, torch.zeros_like(last), (last + first) / 2)
        self.E = torch.where(self.cand, self.eps, torch.zeros_like(self.eps)).amax(dim=-1)
        self.ambiguous = self.cand & ~self.decided[..., None] & ((self.s - cut[..., None]).abs() <= self.eps + self.E[..., None])

    def ambiguous_rows(self):
        """Share of the (b, h, I) rows that hold an ambiguous candidate."""
        return float(self.ambiguous.any(dim=-1).double().mean())


def compare(got, ref: Judged, what=""):
    """The rule of the module docstring.  Returns the share of ambiguous rows."""
    got = got.to(ref.mask.device).bool()
    assert got.shape == ref.mask.shape, (what, tuple(got.shape), tuple(ref.mask.shape))
    free = ref.ambiguous
    wrong = (got != ref.mask) & ~free
    assert not bool(wrong.any()), f"{what}: {int(wrong.sum())} unambiguous blocks differ, first at {wrong.nonzero()[0].tolist()}"
    assert torch.equal(got.sum(dim=-1), ref.mask.sum(dim=-1)), f"{what}: popcount"
    return ref.ambiguous_rows()


def agrees(got, ref: Judged) -> bool:
    try:
        compare(got, ref)
        return True
    except AssertionError:
        return False


def mean_tolerance(x):
    """(fp64 means, elementwise bound of |mean32 - mean64|) for the usp_block_means tests."""
    return block_means(x, with_error=True)
