"""Rates of the block attention mass (profiles/block_mass_rates.txt): B1 H32/4 D128 bf16 causal at S = 16384 and 65536, medians
of interleaved rounds -- every round times each variant once, one after the other.

    python tools/block_mass_rates.py [rounds]

(1) usp_block_attn_mass against (a) the dense two-waves-per-SIMD forward (usp_flash_fwd with USP_FORCE_WAVE32, k_splits 0: the
    kernels of the parent commit, unchanged here) and the default forward on the same GPU, and (b) a torch composition of the
    same function, chunked over heads and row blocks so that no S x S tensor is held;
(2) the worst error against that composition in fp64 on a few heads, as a share of the bound of tests/block_mass_ref.py;
(3) recall: block_mask_recall of BlockSelect(nb / 8) and BlockSelectTopP(0.9) on white noise and on the planted inputs of
    tools/block_select_top_p_rates.py, per head as min / median / max, beside the kept share of the causal blocks."""
import statistics
import sys

import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
sys.path.insert(0, ROOT + "/tools")
import block_mass_ref as MR  # noqa: E402
from block_select_top_p_rates import kept_per_head, planted, timed  # noqa: E402
from yunchang_amd import _C  # noqa: E402
from yunchang_amd.kernels.attention import block_attention_mass, block_mask_recall, select_blocks, select_blocks_top_p  # noqa: E402


def torch_mass(q, k, lse, scale, out, dtype=torch.float32, heads=None, rows_per=2048):
    """The definition as a torch composition (causal; S % 128 == 0), head by head and `rows_per` rows at a time."""
    B, S, Hq, D = q.shape
    G, nb = Hq // k.shape[2], S // 128
    for h in (range(Hq) if heads is None else heads):
        kh = k[0, :, h // G].to(dtype)
        for r0 in range(0, S, rows_per):
            r1 = r0 + rows_per
            s = (q[0, r0:r1, h].to(dtype) @ kh[:r1].T) * scale - lse[0, h, r0:r1, None].to(dtype)
            i = torch.arange(r0, r1, device=q.device)[:, None]
            p = torch.where(torch.arange(r1, device=q.device)[None, :] <= i, torch.exp(s), torch.zeros_like(s))
            out[0, h, r0 // 128:r1 // 128, :r1 // 128] = p.view(rows_per // 128, 128, r1 // 128, 128).sum(dim=(1, 3)) / 128
            out[0, h, r0 // 128:r1 // 128, r1 // 128:] = 0
    return out


def per_head(x):
    v = x[0].flatten(1).double()
    lo, med, hi = v.min(dim=1).values.sort().values, v.median(dim=1).values.sort().values, v.max(dim=1).values.sort().values
    m = v.mean(dim=1).sort().values
    return f"{float(m[0]):.3f} / {float(m[len(m) // 2]):.3f} / {float(m[-1]):.3f} (worst row block of any head {float(lo[0]):.3f})"


def main(rounds=15):
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; B1 H32/4 D128 bf16 causal; {rounds} interleaved rounds behind 2 warm-up rounds, medians in ms")
    for S in (16384, 65536):
        B, Hq, Hkv, D = 1, 32, 4, 128
        nb, scale = S // 128, D ** -0.5
        g = torch.Generator().manual_seed(S)
        q, k, v = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv))
        pq, pk = planted(B, S, Hq, Hkv, D, dev, S + 1)
        out = torch.empty((B, S, Hq, D), dtype=torch.bfloat16, device=dev)
        lse = torch.empty((B, Hq, S), dtype=torch.float32, device=dev)
        plse = torch.empty_like(lse)
        _C.flash_fwd(q, k, v, scale, True, lse, out)
        _C.flash_fwd(pq, pk, pk, scale, True, plse, out)
        mass = torch.empty((B, Hq, nb, nb), dtype=torch.float32, device=dev)
        comp = torch.empty_like(mass)
        variants = {
            "block mass": lambda: _C.block_attn_mass(q, k, lse, scale, True, 0, out=mass),
            "block mass, planted": lambda: _C.block_attn_mass(pq, pk, plse, scale, True, 0, out=mass),
            "forward wave32": lambda: _C.flash_fwd(q, k, v, scale, True, lse, out, family="wave32", k_splits=0),
            "forward default": lambda: _C.flash_fwd(q, k, v, scale, True, lse, out),
            "torch composition": lambda: torch_mass(q, k, lse, scale, comp),
        }
        times = {n: [] for n in variants}
        for r in range(rounds + 2):
            for name, fn in variants.items():
                t = timed(fn)
                if r >= 2:
                    times[name].append(t)
        med = {n: statistics.median(x) for n, x in times.items()}
        tm, tw, td, tc = med["block mass"], med["forward wave32"], med["forward default"], med["torch composition"]
        print(f"S{S}: nb {nb}")
        print(f"  block mass {tm:.4f} (planted {med['block mass, planted']:.4f})")
        print(f"  (a) dense forward, two waves per SIMD {tw:.4f} -> the block mass is {tm / tw:.3f} x of it "
              f"({'NOT slower' if tm <= tw else 'SLOWER'}); default forward {td:.4f} -> {tm / td:.3f} x")
        print(f"  (b) torch composition, chunked over heads and 2048 rows {tc:.4f} -> the block mass is {tm / tc:.3f} x of it")
        _C.block_attn_mass(q, k, lse, scale, True, 0, out=mass)
        heads = [0, 13, 31]
        ref = torch_mass(q, k, lse, scale, torch.zeros((B, Hq, nb, nb), dtype=torch.float64, device=dev), torch.float64, heads)
        worst = 0.0
        for h in heads:
            qh, kh, lh = q[:, :4096, h:h + 1], k[:, :4096, h // 8:h // 8 + 1], lse[:, h:h + 1, :4096]
            d = MR.exponent_error(qh, kh, lh, scale)          # (the exponent's bound from the first 4096 rows and keys of the head)
            err = (mass[:, h:h + 1].double() - ref[:, h:h + 1]).abs() / MR.tolerance(ref[:, h:h + 1], d)
            worst = max(worst, float(err.max()))
        rowsum = mass.double().sum(-1)
        print(f"  worst error on heads {heads} against the fp64 composition: {worst:.4f} of the bound; row sums in "
              f"[{float(rowsum.min()):.7f}, {float(rowsum.max()):.7f}]")
        for name, (a, b, l) in (("white noise", (q, k, lse)), ("planted", (pq, pk, plse))):
            m = block_attention_mass(a, b, l, causal=True)
            for label, mask in ((f"BlockSelect({nb // 8})", select_blocks(a, b, nb // 8, causal=True)),
                                ("BlockSelectTopP(0.9)", select_blocks_top_p(a, b, 0.9, causal=True))):
                rec = block_mask_recall(m, mask)
                print(f"  recall, {name}, {label}: kept share of the causal blocks per head min / median / max "
                      f"{kept_per_head(mask, nb)}; recall per head (mean over row blocks) min / median / max {per_head(rec)}")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 15)
