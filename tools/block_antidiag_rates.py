"""Rates of the antidiagonal block gate (profiles/block_antidiag_rates.txt): B1 H32/4 D128 bf16 causal at S = 16384 and 65536,
medians of interleaved rounds -- every round times each variant once, one after the other, by device events.

    python tools/block_antidiag_rates.py [rounds]

(a) usp_block_antidiag_weights at stride 8 and 16 and usp_block_select_weights alone, against usp_block_attn_mass and against
    pooling + usp_block_select_top_p (the parent commit's kernels, unchanged) in the same run; the weights kernel executes 2 / s of
    the mass kernel's matrix work (two sweeps): the measured ratio stands beside that expectation;
(b) recall: block_mask_recall(block_attention_mass, mask) and the kept share of the causal blocks, per head, on white noise and on
    the planted inputs of tools/block_select_top_p_rates.py, for BlockSelectAntidiag(0.9), BlockSelectTopP(0.9) and BlockSelect at
    the kept share the antidiagonal gate reached;
    and on LINED inputs -- white noise in which one key in 512 (a vertical line) and the key 256 behind every 64th row (a slash
    line) are strong: what a pooled mean dilutes by 128 and an antidiagonal sum by `stride`;
(c) forward + backward of hip_attn_func under BlockSelectAntidiag(0.9) against the dense call."""
import statistics
import sys

import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tools")
from block_mass_rates import per_head  # noqa: E402
from block_select_top_p_rates import kept_per_head, planted, timed  # noqa: E402
from yunchang_amd import BlockSelectAntidiag, _C  # noqa: E402
from yunchang_amd.kernels.attention import (block_attention_mass, block_mask_recall, hip_attn_func, select_blocks,  # noqa: E402
                                            select_blocks_antidiag, select_blocks_from_weights, select_blocks_top_p)


def lined(B, S, Hq, Hkv, D, dev, seed, gain=6.0):
    """White noise with a few strong keys inside the blocks: every query leans towards a direction u; one key in 512 carries
    gain * u (a vertical line: every later row sees it), and so does the key 256 positions behind every 64th row, which leans
    twice as far (a slash line)."""
    g = torch.Generator().manual_seed(seed)
    q, k = (torch.randn(B, S, h, D, generator=g) for h in (Hq, Hkv))
    u = torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0) * D ** 0.5
    q = q + 0.5 * u
    k[:, torch.randperm(S, generator=g)[:S // 512]] += gain * u
    rows = torch.arange(256, S, 64)
    q[:, rows] += 0.5 * u
    k[:, rows - 256] += gain * u
    return q.to(torch.bfloat16).to(dev), k.to(torch.bfloat16).to(dev)


def main(rounds=15):
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; B1 H32/4 D128 bf16 causal; {rounds} interleaved rounds behind 2 warm-up rounds, medians in ms")
    for S in (16384, 65536):
        B, Hq, Hkv, D = 1, 32, 4, 128
        nb, scale = S // 128, D ** -0.5
        g = torch.Generator().manual_seed(S)
        q, k, v, do = (torch.randn(B, S, h, D, generator=g).to(torch.bfloat16).to(dev) for h in (Hq, Hkv, Hkv, Hq))
        pq, pk = planted(B, S, Hq, Hkv, D, dev, S + 1)
        out = torch.empty((B, S, Hq, D), dtype=torch.bfloat16, device=dev)
        lq, lk = lined(B, S, Hq, Hkv, D, dev, S + 2)
        lse, plse, llse = (torch.empty((B, Hq, S), dtype=torch.float32, device=dev) for _ in range(3))
        _C.flash_fwd(q, k, v, scale, True, lse, out)
        _C.flash_fwd(pq, pk, pk, scale, True, plse, out)
        _C.flash_fwd(lq, lk, lk, scale, True, llse, out)
        w = torch.empty((B, Hq, nb, nb), dtype=torch.float32, device=dev)
        mass = torch.empty_like(w)
        mask = torch.empty((B, Hq, nb, nb), dtype=torch.bool, device=dev)
        tq, tk, tv = (t.clone().requires_grad_(True) for t in (q, k, v))

        def step(**kw):
            hip_attn_func(tq, tk, tv, causal=True, **kw).backward(do)
        variants = {
            "weights s8": lambda: _C.block_antidiag_weights(q, k, scale, True, 8, out=w),
            "weights s16": lambda: _C.block_antidiag_weights(q, k, scale, True, 16, out=w),
            "selector": lambda: _C.block_select_weights(w, 0.9, True, 0, 1, 0, out=mask),
            "block mass": lambda: _C.block_attn_mass(q, k, lse, scale, True, 0, out=mass),
            "pool + top-p": lambda: _C.block_select_top_p(_C.block_means(q), _C.block_means(k), 0.9, scale, True, 0, 1, False, 0, out=mask),
            "fwd+bwd antidiag": lambda: step(block_select=BlockSelectAntidiag(0.9)),
            "fwd+bwd dense": lambda: step(),
        }
        times = {n: [] for n in variants}
        for r in range(rounds + 2):
            for name, fn in variants.items():
                t = timed(fn)
                if r >= 2:
                    times[name].append(t)
        med = {n: statistics.median(x) for n, x in times.items()}
        tm = med["block mass"]
        print(f"S{S}: nb {nb}")
        for s in (8, 16):
            t = med[f"weights s{s}"]
            print(f"  (a) weights, stride {s}: {t:.4f}; block mass {tm:.4f}: measured ratio {t / tm:.3f} against {2 / s:.3f} of its matrix "
                  f"work -- {'faster than the mass kernel' if t < tm else '**NOT faster than the mass kernel**'}")
        print(f"  (a) selector alone {med['selector']:.4f}; pooling + usp_block_select_top_p {med['pool + top-p']:.4f}")
        ta, td = med["fwd+bwd antidiag"], med["fwd+bwd dense"]
        print(f"  (c) forward + backward: BlockSelectAntidiag(0.9) {ta:.4f}, dense {td:.4f} -> {ta / td:.3f} x "
              f"({'faster' if ta < td else '**slower than the dense call**'})")
        for name, (a, b, l) in (("white noise", (q, k, lse)), ("planted", (pq, pk, plse)), ("lined", (lq, lk, llse))):
            m = block_attention_mass(a, b, l, causal=True)
            anti = select_blocks_antidiag(a, b, 0.9, causal=True)
            print(f"  (b) {name}, the map itself as the selector, select_blocks_from_weights(block_attention_mass, 0.9): kept "
                  f"{kept_per_head(select_blocks_from_weights(m, 0.9, causal=True), nb)}")
            kept = float(anti.sum()) / (Hq * nb * (nb + 1) / 2)
            top_k = max(1, round(kept * (nb + 1) / 2))               # the mean count of kept blocks per row block
            for label, msk in (("BlockSelectAntidiag(0.9)", anti), ("BlockSelectTopP(0.9)", select_blocks_top_p(a, b, 0.9, causal=True)),
                               (f"BlockSelect({top_k})", select_blocks(a, b, top_k, causal=True))):
                print(f"  (b) {name}, {label}: kept share of the causal blocks per head min / median / max {kept_per_head(msk, nb)}; "
                      f"recall per head (mean over row blocks) min / median / max {per_head(block_mask_recall(m, msk))}")
    print("multi-GPU: not measured.  The register, spill and kernel_isa lines below this one are not printed by this tool: they are read off the code\n"
          "object metadata (llvm-readelf --notes) and tools/kernel_isa.py --every and appended by hand.")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 15)
