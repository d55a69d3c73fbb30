"""Rates of the top-p block selection (profiles/block_select_top_p_rates.txt): B1 H32/4 D128 bf16 causal at S = 16384 and 65536,
medians of interleaved rounds -- every round times each variant once, one after the other.

    python tools/block_select_top_p_rates.py [rounds]

(1) pooling + top-p selection (usp_block_means twice, usp_block_select_top_p) against (a) the torch composition of the same
    function on the same GPU (reshape, mean, einsum, softmax, sort, cumsum, scatter) and (b) pooling + the top-k selection at
    top_k = nb / 8; with share_group beside it;
(2) the kept share of the causal blocks per head -- minimum / median / maximum over the 32 heads -- at top_p 0.9 and 0.95, on
    white noise and on planted inputs (every key block its own direction; a row block of head h points at block 0, at three
    blocks of its past and faintly at the rest, times a temperature that grows with h: peaked heads and diffuse ones);
(3) end to end, forward + backward through hip_attn_func: block_select=BlockSelectTopP(0.9) against the dense call, on both."""
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import yunchang_amd as Y  # noqa: E402
from yunchang_amd import _C  # noqa: E402
from yunchang_amd.kernels.attention import hip_attn_func, select_blocks, select_blocks_top_p  # noqa: E402


def torch_select_top_p(q, k, top_p, scale, I, J):
    """The definition as a torch composition on the operands' device (causal, keep_first = 0, keep_local = 1; S % 128 == 0)."""
    B, S, Hq, D = q.shape
    Hkv, nb = k.shape[2], S // 128
    qbar = q.float().view(B, nb, 128, Hq, D).mean(2)
    kbar = k.float().view(B, nb, 128, Hkv, D).mean(2).repeat_interleave(Hq // Hkv, dim=2)
    s = torch.einsum("bihd,bjhd->bhij", qbar, kbar) * scale
    w = torch.softmax(torch.where(J <= I, s, torch.full_like(s, float("-inf"))), dim=-1)
    forced, cand = J == I, J < I
    mass_f = torch.where(forced, w, torch.zeros_like(w)).sum(dim=-1, keepdim=True)
    sw, order = torch.where(cand, w, torch.full_like(w, -1.0)).sort(dim=-1, descending=True, stable=True)
    sw = sw.clamp(min=0)
    take = (mass_f + sw.cumsum(dim=-1) - sw) < top_p                      # the mass in front of a block has not reached top_p
    sel = torch.zeros_like(take).scatter_(-1, order, take)
    return forced | (cand & sel)


def planted(B, S, Hq, Hkv, D, dev, seed):
    g = torch.Generator().manual_seed(seed)
    nb, G = S // 128, Hq // Hkv
    dirs = torch.nn.functional.normalize(torch.randn(Hkv, nb, D, generator=g), dim=-1)
    k = dirs.permute(1, 0, 2).repeat_interleave(128, dim=0)[None] + 0.05 * torch.randn(B, S, Hkv, D, generator=g)
    I = torch.arange(nb)
    q = torch.empty(B, nb, Hq, D)
    for h in range(Hq):
        d = dirs[h // G]
        hot = d[0][None] + d[(I - 3).clamp(min=0)] + d[I // 2] + d[(I * 3) // 4] + 0.3 * d.mean(0, keepdim=True) * nb ** 0.5
        q[0, :, h] = hot * (4.0 * 2.0 ** (h / 4.0))                       # temperature 4 .. 860 over the heads
    q = q.repeat_interleave(128, dim=1) + 0.05 * torch.randn(B, S, Hq, D, generator=g)
    return q.to(torch.bfloat16).to(dev), k.to(torch.bfloat16).to(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kept_per_head(mask, nb):
    causal = nb * (nb + 1) / 2
    share = (mask[0].flatten(1).sum(dim=1).double() / causal).sort().values
    return f"{float(share[0]):.3f} / {float(share[len(share) // 2]):.3f} / {float(share[-1]):.3f}"


def main(rounds=15):
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; B1 H32/4 D128 bf16 causal; {rounds} interleaved rounds behind 2 warm-up rounds, medians in ms")
    for S in (16384, 65536):
        B, Hq, Hkv, D = 1, 32, 4, 128
        nb, scale = S // 128, D ** -0.5
        top_k = nb // 8
        g = torch.Generator().manual_seed(S)
        q, k, v, do = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv, Hq))
        pq, pk = planted(B, S, Hq, Hkv, D, dev, S + 1)
        I, J = torch.arange(nb, device=dev)[:, None], torch.arange(nb, device=dev)[None, :]
        qbar, kbar = _C.block_means(q), _C.block_means(k)
        pqbar, pkbar = _C.block_means(pq), _C.block_means(pk)
        mask = torch.empty((B, Hq, nb, nb), dtype=torch.bool, device=dev)
        variants = {
            "pool q+k": lambda: (_C.block_means(q, out=qbar), _C.block_means(k, out=kbar)),
            "top-p select": lambda: _C.block_select_top_p(qbar, kbar, 0.9, scale, True, 0, 1, False, 0, out=mask),
            "top-p select, share_group": lambda: _C.block_select_top_p(qbar, kbar, 0.9, scale, True, 0, 1, True, 0, out=mask),
            "top-p select, planted": lambda: _C.block_select_top_p(pqbar, pkbar, 0.9, scale, True, 0, 1, False, 0, out=mask),
            "top-k select": lambda: _C.block_select(qbar, kbar, top_k, scale, True, 0, 1, 0, out=mask),
            "select_blocks_top_p": lambda: select_blocks_top_p(q, k, 0.9, causal=True),
            "select_blocks (top-k)": lambda: select_blocks(q, k, top_k, causal=True),
            "torch composition": lambda: torch_select_top_p(q, k, 0.9, scale, I, J),
        }
        print(f"S{S}: nb {nb}")
        for name, (a, b) in (("white noise", (q, k)), ("planted", (pq, pk))):
            for p in (0.9, 0.95):
                got = select_blocks_top_p(a, b, p, causal=True)
                differ = int((got != torch_select_top_p(a, b, p, scale, I, J)).sum())
                shared = select_blocks_top_p(a, b, p, causal=True, share_group=True)
                print(f"  kept share of the causal blocks per head, min / median / max, {name}, top_p {p}: {kept_per_head(got, nb)}"
                      f"  (share_group: {kept_per_head(shared, nb)}); blocks that differ from the torch composition (fp32 sums in "
                      f"another order): {differ} of {got.numel()}")

        def step(a, b, **kw):
            lq, lk, lv = (t.detach().requires_grad_(True) for t in (a, b, v))
            hip_attn_func(lq, lk, lv, causal=True, **kw).backward(do)
        e2e = {"dense": lambda: step(q, k), "block_select=BlockSelectTopP(0.9), white noise": lambda: step(q, k, block_select=Y.BlockSelectTopP(0.9)),
               "dense, planted": lambda: step(pq, pk),
               "block_select=BlockSelectTopP(0.9), planted": lambda: step(pq, pk, block_select=Y.BlockSelectTopP(0.9))}
        times = {n: [] for n in list(variants) + list(e2e)}
        for r in range(rounds + 2):
            for name, fn in list(variants.items()) + list(e2e.items()):
                t = timed(fn)
                if r >= 2:
                    times[name].append(t)
        med = {n: statistics.median(x) for n, x in times.items()}
        tp, tk, tc = med["select_blocks_top_p"], med["select_blocks (top-k)"], med["torch composition"]
        print(f"  pool q+k {med['pool q+k']:.4f}  top-p select {med['top-p select']:.4f} (share_group {med['top-p select, share_group']:.4f}, "
              f"planted {med['top-p select, planted']:.4f})  top-k select (top_k {top_k}) {med['top-k select']:.4f} -> "
              f"{med['top-p select'] / med['top-k select']:.2f} x the top-k kernel")
        print(f"  select_blocks_top_p (pooling + selection, with allocation) {tp:.4f}")
        print(f"  (a) torch composition {tc:.4f} -> select_blocks_top_p is {tp / tc:.2f} x of it ({'NOT slower' if tp <= tc else 'SLOWER'})")
        print(f"  (b) select_blocks at top_k = nb / 8 {tk:.4f} -> select_blocks_top_p is {tp / tk:.2f} x of it")
        for tag in ("white noise", "planted"):
            d = med["dense" if tag == "white noise" else "dense, planted"]
            s = med[f"block_select=BlockSelectTopP(0.9), {tag}"]
            print(f"  end to end fwd+bwd, {tag}: dense {d:.3f}  block_select=BlockSelectTopP(0.9) {s:.3f} ({s / d:.3f} x dense)")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 15)
