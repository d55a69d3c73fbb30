"""Rates of the block selection (profiles/block_select_rates.txt): B1 H32/4 D128 bf16 causal at S = 16384 and 65536, top_k = nb / 8,
medians of interleaved rounds -- every round times each variant once, one after the other.

    python tools/block_select_rates.py [rounds]

(1) pooling + selection (usp_block_means twice, usp_block_select) against (a) the torch composition of the same function on the
    same GPU (reshape, mean, einsum, stable sort, scatter: the reference implementation moved to the device) and (b) the dense
    two-waves-per-SIMD forward of the shape; the pooling kernel's bytes per second against the nominal 8 TB/s of HBM;
(2) end to end, forward + backward through hip_attn_func: block_select=BlockSelect(nb // 8) against the dense call and against the
    block_mask= call with the mask precomputed."""
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import yunchang_amd as Y  # noqa: E402
from yunchang_amd import _C  # noqa: E402
from yunchang_amd.kernels.attention import hip_attn_func, select_blocks  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def torch_select(q, k, top_k, scale, I, J):
    """The definition as a torch composition on the operands' device (causal, keep_first = 0, keep_local = 1; S % 128 == 0)."""
    B, S, Hq, D = q.shape
    Hkv, nb = k.shape[2], S // 128
    qbar = q.float().view(B, nb, 128, Hq, D).mean(2)
    kbar = k.float().view(B, nb, 128, Hkv, D).mean(2).repeat_interleave(Hq // Hkv, dim=2)
    s = torch.einsum("bihd,bjhd->bhij", qbar, kbar) * scale
    forced = J == I
    cand = J < I
    key = torch.where(cand, s, torch.full_like(s, float("-inf")))
    order = key.sort(dim=-1, descending=True, stable=True).indices
    rank = torch.empty_like(order)
    rank.scatter_(-1, order, J.expand_as(order).contiguous())
    return forced | (cand & (rank < top_k - 1))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main(rounds=15):
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; B1 H32/4 D128 bf16 causal; {rounds} interleaved rounds behind 2 warm-up rounds, medians in ms")
    for S in (16384, 65536):
        B, Hq, Hkv, D = 1, 32, 4, 128
        nb, scale = S // 128, D ** -0.5
        top_k = nb // 8
        g = torch.Generator().manual_seed(S)
        q, k, v, do = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv, Hq))
        I, J = torch.arange(nb, device=dev)[:, None], torch.arange(nb, device=dev)[None, :]
        qbar, kbar = _C.block_means(q), _C.block_means(k)
        mask = torch.empty((B, Hq, nb, nb), dtype=torch.bool, device=dev)
        out, lse = torch.empty_like(q), torch.empty((B, Hq, S), dtype=torch.float32, device=dev)
        variants = {
            "pool q+k": lambda: (_C.block_means(q, out=qbar), _C.block_means(k, out=kbar)),
            "select": lambda: _C.block_select(qbar, kbar, top_k, scale, True, 0, 1, 0, out=mask),
            "select_blocks": lambda: select_blocks(q, k, top_k, causal=True),
            "torch composition": lambda: torch_select(q, k, top_k, scale, I, J),
            "dense forward": lambda: _C.flash_fwd(q, k, v, scale, True, lse, out=out, k_splits=0, family="wave32"),
        }
        pre = select_blocks(q, k, top_k, causal=True)
        differ = int((pre != torch_select(q, k, top_k, scale, I, J)).sum())

        def step(**kw):
            lq, lk, lv = (t.detach().requires_grad_(True) for t in (q, k, v))
            hip_attn_func(lq, lk, lv, causal=True, **kw).backward(do)
        e2e = {"dense": lambda: step(), "block_mask= (precomputed)": lambda: step(block_mask=pre),
               "block_select=": lambda: step(block_select=Y.BlockSelect(top_k))}
        times = {n: [] for n in list(variants) + list(e2e)}
        for r in range(rounds + 2):
            for name, fn in list(variants.items()) + list(e2e.items()):
                t = timed(fn)
                if r >= 2:
                    times[name].append(t)
        med = {n: statistics.median(x) for n, x in times.items()}
        pool_bytes = (q.numel() + k.numel()) * 2 + (qbar.numel() + kbar.numel()) * 4
        kept = float(pre.sum()) / float(torch.tril(torch.ones(nb, nb)).sum() * B * Hq)
        print(f"S{S}: nb {nb}, top_k {top_k}; the selection keeps {kept:.4f} of the causal blocks; blocks that differ from the torch "
              f"composition (fp32 sums in another order): {differ} of {pre.numel()}")
        print(f"  pool q+k {med['pool q+k']:.4f} ({pool_bytes / (med['pool q+k'] * 1e-3) / 1e9:.0f} GB/s = "
              f"{pool_bytes / (med['pool q+k'] * 1e-3) / HBM_BYTES_PER_S:.2f} of 8 TB/s)  select {med['select']:.4f}  "
              f"select_blocks (both, with allocation) {med['select_blocks']:.4f}")
        print(f"  (a) torch composition {med['torch composition']:.4f} -> select_blocks is {med['select_blocks'] / med['torch composition']:.2f} x "
              f"of it ({'NOT slower' if med['select_blocks'] <= med['torch composition'] else 'SLOWER'})")
        print(f"  (b) dense two-waves-per-SIMD forward {med['dense forward']:.3f} -> select_blocks is "
              f"{med['select_blocks'] / med['dense forward']:.4f} x of it")
        print(f"  end to end fwd+bwd: dense {med['dense']:.3f}  block_mask= (precomputed) {med['block_mask= (precomputed)']:.3f}  "
              f"block_select= {med['block_select=']:.3f} ({med['block_select='] / med['dense']:.3f} x dense, "
              f"+{med['block_select='] - med['block_mask= (precomputed)']:.3f} ms over the precomputed mask)")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 15)
