"""The reference of the top-p block selection (`block_select=BlockSelectTopP(...)`, kernels/attention.py: select_blocks_top_p;
include/usp_hip.h: usp_block_select_top_p), in fp64, written from the definition alone -- nothing of the package is imported
(tests/block_select_ref.py lends block_means, scores, score_eps and candidates):

    score, visible, forced: those of the top-k selection (tests/block_select_ref.py), I the GLOBAL row block
    w[J] = exp(score[J] - m) / Z over the VISIBLE blocks (m their maximum, Z their sum), 0 elsewhere
    selected = forced + the SHORTEST prefix of the other visible blocks by (w descending, J ascending) with
               mass(forced) + mass(prefix) >= top_p   (no prefix where the forced blocks reach top_p)
    share_group: w = the mean over the G query heads of a KV head of their per-head w; one row for the group

The mutants of tests/test_block_select_top_p_cpu.py are arguments here (`mutant=`), so the unmutated path is the one the GPU tests
use.

The tolerance is derived, not chosen.  The kernel works in fp32 (u = 2^-24) in the order include/usp_hip.h documents.
  * a score: |score32 - score64| <= eps_s (tests/block_select_ref.py: score_eps).  The row maximum is exact on the fp32 scores,
    and its own error is a factor common to every exponential and to Z: it cancels in e / Z.
  * an exponential e[J] = expf(score[J] - m): the subtraction rounds once, u |score - m| in the argument; expf itself has the
    relative error EXP_REL.  ROCm ships no document that states a bound for the function called (OCML's __ocml_exp_f32,
    what hipcc makes of expf without fast-math), so it was MEASURED alone against fp64 on an MI355X over every
    fp32 argument in [-126 ln 2, 0] (1.1e9 of them): the largest relative error is 8.4091e-08, 0.705 ulp, at x = -42.9318275 (EXP_MEASURED), and EXP_REL is twice
    that.  Command:
        hipcc --offload-arch=gfx950 -O3 tools/expf_error.hip -o expf_error && ./expf_error
    (profiles/block_select_top_p_rates.txt keeps its output.)  Below -126 ln 2 the result may be flushed: an absolute 2^-125.
    To first order the relative error of e[J] is r[J] = eps_s[J] + u |score[J] - m| + EXP_REL.
  * Z and every mass: SUM adds a term through at most L = ceil(nbk / 256) - 1 + 6 + 3 additions (a thread's stride, the wave's
    butterfly, the four waves), so for non-negative terms |SUM32 - SUM| <= L u SUM; Z also carries its terms' errors,
    sum_J w[J] r[J] relative.
  * the division e / Z rounds once (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt): u.
    eps[J] = (w[J] (r[J] + sum_J' w[J'] r[J'] + L u + u)) (1 + 2^-10) + 2^-125
  * share_group: the G heads' weights are added in ascending order, G - 1 roundings of partial sums below the total:
    eps[J] = mean_g eps_g[J] + (G - 1) u wbar[J]   (the kernel's sum over heads is G times the mean; only ratios enter the rule).
  * the rule compares mass32(set) with fl(top_p32 * total32): the two sums (2 L u), the product, top_p's own rounding to fp32,
    and the fused multiply-add of the tie expression (u each):  E = sum_J eps[J] + (2 L + 4) u.

The acceptance rule (`passes`): with these eps and E a kernel row G passes iff
  1. forced <= G <= visible;
  2. no selected non-forced a and rejected visible b have w[a] + eps[a] < w[b] - eps[b]; where w[a] == w[b] exactly, the lower J
     comes first (no rejected b below a selected a of the same weight);
  3. mass(G) >= top_p - E, or G is everything visible;
  4. G has no non-forced member, or mass(G) - (the smallest w among them) < top_p + E.
Under share_group the rows of a group's heads must be identical and pass against the group's mean weights.

A row is AMBIGUOUS when more than one set passes; `ambiguous_rows` tries the three nearest neighbours of the reference's set --
its prefix one shorter, one longer, and the last selected swapped for the first rejected -- which every other passing set
implies one of (a set that passes differs from the reference's by blocks within eps of the cut or by mass within E)."""
import torch

import block_select_ref as SR

BLOCK = SR.BLOCK
U = SR.U
EXP_MEASURED = 8.4091e-08
EXP_REL = 2 * EXP_MEASURED
TINY = 2.0 ** -125
MUTANTS = ("mass_without_forced", "softmax_all_blocks", "count_share", "one_short", "one_long", "tie_high", "wrong_kv_head",
           "drop_row_offset", "share_avg_scores", "share_unnormalised")


def depth(nbk):
    """Additions a term of SUM passes through."""
    return (nbk + 255) // 256 - 1 + 6 + 3


def softmax_visible(s, vis):
    """(w, m): the softmax of fp64 scores (.., nbq, nbk) over the blocks `vis` (nbq, nbk) marks, 0 elsewhere."""
    neg = torch.full_like(s, float("-inf"))
    sm = torch.where(vis, s, neg)
    m = sm.amax(dim=-1, keepdim=True)
    e = torch.where(vis, torch.exp(sm - m), torch.zeros_like(s))
    return e / e.sum(dim=-1, keepdim=True), m


def weights(s, visible, Hkv, share=False, mutant=None):
    """fp64 (B, Hq, nbq, nbk) weights from scores of that shape."""
    vis = torch.ones_like(visible) if mutant == "softmax_all_blocks" else visible
    B, Hq, nbq, nbk = s.shape
    G = Hq // Hkv
    if share and mutant == "share_avg_scores":
        s = s.view(B, Hkv, G, nbq, nbk).mean(dim=2, keepdim=True).expand(B, Hkv, G, nbq, nbk).reshape(B, Hq, nbq, nbk)
    w, m = softmax_visible(s, vis)
    w = torch.where(visible, w, torch.zeros_like(w))
    if share and mutant == "share_unnormalised":
        e = torch.where(visible, torch.exp(torch.where(visible, s, torch.full_like(s, float("-inf"))) - m), torch.zeros_like(s))
        e = e.view(B, Hkv, G, nbq, nbk).sum(dim=2, keepdim=True)
        w = (e / e.sum(dim=-1, keepdim=True)).expand(B, Hkv, G, nbq, nbk).reshape(B, Hq, nbq, nbk)
    elif share and mutant != "share_avg_scores":
        w = w.view(B, Hkv, G, nbq, nbk).mean(dim=2, keepdim=True).expand(B, Hkv, G, nbq, nbk).reshape(B, Hq, nbq, nbk)
    return w


def order_of(w, cand, tie_high=False):
    """(order, rank): the blocks of a row by (candidates first, w descending, J ascending) and each block's place in it."""
    nbk = w.shape[-1]
    key = torch.where(cand, -w, torch.full_like(w, float("inf")))
    if tie_high:
        order = nbk - 1 - key.flip(-1).sort(dim=-1, stable=True).indices
    else:
        order = key.sort(dim=-1, stable=True).indices
    rank = torch.empty_like(order)
    rank.scatter_(-1, order, torch.arange(nbk, device=w.device).expand_as(order).contiguous())
    return order, rank


def select_from_weights(w, top_p, visible, forced, mutant=None):
    """bool mask from fp64 weights (B, Hq, nbq, nbk) and (nbq, nbk) visible / forced."""
    cand = (visible & ~forced).expand_as(w)
    forced = forced.expand_as(w)
    order, rank = order_of(w, cand, mutant == "tie_high")
    zero = torch.zeros_like(w)
    mass_f = zero[..., 0] if mutant == "mass_without_forced" else torch.where(forced, w, zero).sum(dim=-1)
    sorted_w = torch.where(cand, w, zero).gather(-1, order)
    cs = mass_f[..., None] + sorted_w.cumsum(dim=-1)
    n_cand = cand.sum(dim=-1)
    reached = cs >= top_p
    first = torch.where(reached.any(dim=-1), reached.to(torch.int64).argmax(dim=-1) + 1, n_cand)
    k = torch.where(mass_f >= top_p, torch.zeros_like(first), torch.minimum(first, n_cand))
    if mutant == "count_share":
        k = (torch.ceil(top_p * visible.sum(dim=-1).double()).long() - forced.sum(dim=-1)).clamp(min=0)
        k = torch.minimum(k.expand_as(n_cand), n_cand)
    if mutant == "one_short":
        k = (k - 1).clamp(min=0)
    if mutant == "one_long":
        k = torch.minimum(k + 1, n_cand)
    return forced | (cand & (rank < k[..., None]))


def select_ref(q, k, top_p, scale=None, causal=False, keep_first=0, keep_local=1, share=False, mutant=None):
    """The whole-sequence reference mask, bool (B, Hq, nb, nb)."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    inner = mutant if mutant in SR.MUTANTS else None
    s = SR.scores(SR.block_means(q), SR.block_means(k), scale, inner)
    nb = s.shape[-1]
    visible, forced = SR.candidates(nb, nb, causal, keep_first, keep_local, 0, inner)
    return select_from_weights(weights(s, visible, k.shape[2], share, mutant), top_p, visible, forced, mutant)


def select_from_means(qbar, kbar, top_p, scale, causal=False, keep_first=0, keep_local=1, share=False, row_block0=0, mutant=None):
    """What a call of the entry point selects: bool (B, Hq, nbq, nbk) from means (B, nbq, Hq, D), (B, nbk, Hkv, D)."""
    inner = mutant if mutant in SR.MUTANTS else None
    s = SR.scores(qbar, kbar, scale, inner)
    visible, forced = SR.candidates(s.shape[-2], s.shape[-1], causal, keep_first, keep_local, row_block0, inner, s.device)
    return select_from_weights(weights(s, visible, kbar.shape[2], share, mutant), top_p, visible, forced, mutant)


def select_ref_rows(q, k, top_p, scale, causal, keep_first, keep_local, share, P, r, mutant=None):
    """What ring rank r of P selects: its rows of the whole sequence against all key blocks, bool (B, Hq, n, nb)."""
    n = SR.n_blocks(q.shape[1]) // P
    qbar = SR.block_means(q[:, r * n * BLOCK:(r + 1) * n * BLOCK])
    return select_from_means(qbar, SR.block_means(k), top_p, scale, causal, keep_first, keep_local, share, r * n, mutant)


class Problem:
    """The fp64 scores and their error bounds of one (q, k, scale) or of given means: what every selection of it is judged from."""

    def __init__(self, q=None, k=None, scale=None, means=None):
        if means is None:
            self.scale = q.shape[-1] ** -0.5 if scale is None else scale
            self.qbar, eq = SR.block_means(q, with_error=True)
            self.kbar, ek = SR.block_means(k, with_error=True)
        else:                                                      # fp32 means handed to the entry point: exact
            self.scale = scale
            self.qbar, self.kbar = means[0].double(), means[1].double()
            eq, ek = torch.zeros_like(self.qbar), torch.zeros_like(self.kbar)
        self.Hkv = self.kbar.shape[2]
        self.s = SR.scores(self.qbar, self.kbar, self.scale)
        self.eps_s = SR.score_eps(self.qbar, eq, self.kbar, ek, self.scale)

    def judge(self, top_p, causal=False, keep_first=0, keep_local=1, share=False, row_block0=0):
        return Judged(self, top_p, causal, keep_first, keep_local, share, row_block0)


class Judged:
    """One selection of a problem: the reference mask, the weights, eps (B, Hq, nbq, nbk) and E (B, Hq, nbq)."""

    def __init__(self, problem, top_p, causal=False, keep_first=0, keep_local=1, share=False, row_block0=0):
        s = problem.s
        B, Hq, nbq, nbk = s.shape
        self.top_p, self.share, self.G = float(top_p), bool(share), Hq // problem.Hkv
        self.visible, self.forced = SR.candidates(nbq, nbk, causal, keep_first, keep_local, row_block0, None, s.device)
        self.cand = (self.visible & ~self.forced).expand_as(s)
        w, m = softmax_visible(s, self.visible)
        zero = torch.zeros_like(w)
        L = depth(nbk)
        r = torch.where(self.visible, problem.eps_s + U * (s - m).abs() + EXP_REL, zero)
        eps = (w * (r + (w * r).sum(dim=-1, keepdim=True) + L * U + U)) * (1 + 2.0 ** -10) + torch.where(self.visible, zero + TINY, zero)
        if share:
            G, Hkv = self.G, problem.Hkv
            mean = lambda t: t.view(B, Hkv, G, nbq, nbk).mean(dim=2, keepdim=True).expand(B, Hkv, G, nbq, nbk).reshape(B, Hq, nbq, nbk)
            w = mean(w)
            eps = mean(eps) + (G - 1) * U * w
        self.w, self.eps = w, eps
        self.E = eps.sum(dim=-1) + (2 * L + 4) * U
        self.mask = select_from_weights(w, self.top_p, self.visible, self.forced)

    def passes(self, got):
        """bool (B, Hq, nbq): which rows of `got` pass the acceptance rule."""
        w, eps, cand = self.w, self.eps, self.cand
        inf = torch.full_like(w, float("inf"))
        ok = ~((self.forced & ~got) | (got & ~self.visible)).any(dim=-1)                          # 1
        sel, rej = got & cand, ~got & cand
        ok &= ~(torch.where(sel, w + eps, inf).amin(dim=-1) < torch.where(rej, w - eps, -inf).amax(dim=-1))   # 2
        # 2, exact ties: sorted by (w, J), no rejected block stands in front of a selected one of its run of equal weights
        ws, idx = torch.where(cand, w, -inf).sort(dim=-1, stable=True)
        sel_s, rej_s = sel.gather(-1, idx), rej.gather(-1, idx)
        pos = torch.arange(w.shape[-1], device=w.device).expand_as(idx)
        run = torch.cat([torch.zeros_like(pos[..., :1]), (ws[..., 1:] != ws[..., :-1]).long().cumsum(dim=-1)], dim=-1)
        last_sel = torch.full_like(pos, -1).scatter_reduce(-1, run, torch.where(sel_s, pos, torch.full_like(pos, -1)), "amax")
        ok &= ~(rej_s & (last_sel.gather(-1, run) > pos)).any(dim=-1)
        mass = torch.where(got, w, torch.zeros_like(w)).sum(dim=-1)
        ok &= (mass >= self.top_p - self.E) | (got == self.visible).all(dim=-1)                   # 3
        ok &= ~sel.any(dim=-1) | (mass - torch.where(sel, w, inf).amin(dim=-1) < self.top_p + self.E)   # 4
        return ok

    def neighbours(self):
        """The reference's set with its prefix one shorter, one longer, and its last block swapped for the next: three masks and,
        for each, which rows it differs from the reference in."""
        order, rank = order_of(self.w, self.cand)
        k = (self.mask & self.cand).sum(dim=-1, keepdim=True)
        n_cand = self.cand.sum(dim=-1, keepdim=True)
        last, nxt = self.cand & (rank == k - 1), self.cand & (rank == k) & (k < n_cand)
        short, long_ = self.mask & ~last, self.mask | nxt
        swap = torch.where(nxt.any(dim=-1, keepdim=True) & last.any(dim=-1, keepdim=True), (self.mask & ~last) | nxt, self.mask)
        return [(m, (m != self.mask).any(dim=-1)) for m in (short, long_, swap)]

    def ambiguous(self):
        """bool (B, Hq, nbq): rows where another set than the reference's passes."""
        amb = torch.zeros_like(self.E, dtype=torch.bool)
        for m, differs in self.neighbours():
            amb |= differs & self.passes(m)
        return amb

    def ambiguous_rows(self):
        return float(self.ambiguous().double().mean())

    def counts(self):
        """(selected blocks, visible blocks) per row."""
        return self.mask.sum(dim=-1), self.visible.sum(dim=-1).expand_as(self.E)


def compare(got, ref: Judged, what=""):
    """The acceptance rule over every row (and, under share_group, one row per group).  Returns the share of ambiguous rows."""
    got = got.to(ref.mask.device).bool()
    assert got.shape == ref.mask.shape, (what, tuple(got.shape), tuple(ref.mask.shape))
    ok = ref.passes(got)
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} rows fail the rule, first at {(~ok).nonzero()[0].tolist()}"
    if ref.share:
        B, Hq, nbq, nbk = got.shape
        grp = got.view(B, Hq // ref.G, ref.G, nbq, nbk)
        assert bool((grp == grp[:, :, :1]).all()), f"{what}: the heads of a group differ"
    return ref.ambiguous_rows()


def agrees(got, ref: Judged) -> bool:
    try:
        compare(got, ref)
        return True
    except AssertionError:
        return False


# ---- the kernel's SUM in fp32, for the cases that are exact by construction ------------------------------------------------------
def sum32(x):
    """SUM of include/usp_hip.h over a 1-D fp32 tensor, the same bits: a thread's stride ascending, the butterfly, the waves."""
    x = x.to(torch.float32)
    n = x.numel()
    pad = (-n) % 256
    x = torch.cat([x, torch.zeros(pad, dtype=torch.float32)]).view(-1, 256)
    acc = torch.zeros(256, dtype=torch.float32)
    for row in x:
        acc = acc + row
    acc = acc.view(4, 64)
    for half in (32, 16, 8, 4, 2, 1):
        acc = acc.view(4, -1, 2, half)
        acc = (acc[:, :, 0] + acc[:, :, 1]).reshape(4, -1)
    acc = acc.view(4)
    return ((acc[0] + acc[1]) + acc[2]) + acc[3]


def equal_weight_count(n_visible, forced_row, top_p):
    """How many non-forced blocks a row of n_visible EQUAL scores selects, by the kernel's own arithmetic (include/usp_hip.h: the
    tie expression): every weight is wt = fl(1 / n_visible) (e = 1, Z = n_visible exactly), the cut is that weight's key,
    m_gt = SUM(forced weights), target = fl(fl(top_p) * SUM(all weights)), need = the smallest c with fmaf(c, wt, m_gt) >=
    target.  `forced_row`: bool (nbk,)."""
    f32 = torch.float32
    nbk = forced_row.numel()
    wt = (torch.ones((), dtype=f32) / torch.tensor(float(n_visible), dtype=f32))
    wrow = torch.zeros(nbk, dtype=f32)
    wrow[:n_visible] = wt
    total = sum32(wrow)
    target = torch.tensor(top_p, dtype=f32) * total
    m_gt = sum32(torch.where(forced_row, wrow, torch.zeros_like(wrow)))
    n_eq = n_visible - int(forced_row[:n_visible].sum())
    if m_gt >= target:
        return 0
    for c in range(1, n_eq + 1):
        fma = torch.tensor(c * float(wt) + float(m_gt), dtype=torch.float64).to(f32)     # (exact in fp64, rounded once: fmaf)
        if fma >= target:
            return c
    return n_eq
