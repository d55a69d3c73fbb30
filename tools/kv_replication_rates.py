"""DEV TOOL (one GPU): achieved HBM rate of the dK/dV return of a Ulysses exchange whose KV heads are shared by r ranks
(usp_sum_rows through comm/all_to_all.py:unpack_kv_sum), beside usp_copy_rows moving the same rows (the unpack of an
exchange without replication).  Default shape: one rank of the 8 x 1 grid at bench.py's 64K workload (H32 / Hkv4 D128 bf16):
the receive buffer holds 8 chunks x 8192 rows x (dk | dv) x 128 x 2 B; each of the two launches reads 8 chunks of one head and
writes 4 KV heads.  Device events around `--iters` back-to-back launch pairs; bytes = read + written.

    python tools/kv_replication_rates.py [--P 8] [--hkv 4] [--rows 8192] [--iters 50]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=8)
    ap.add_argument("--hkv", type=int, default=4)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    import yunchang_amd.comm.all_to_all as A
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    P, Hkv, Sl, D, B = args.P, args.hkv, args.rows, args.D, 1
    r = A.kv_replicas(Hkv, P)
    assert r > 1, "the KV heads must be shared (Hkv < P, P % Hkv == 0)"
    recv = torch.randn(P, Sl, B, 2, D, device=dev).to(torch.bfloat16)            # chunk p: rank p's dk | dv partials
    dk = torch.empty(B, Sl, Hkv, D, device=dev, dtype=torch.bfloat16)
    dv = torch.empty_like(dk)

    def reduce_pair():
        A.unpack_kv_sum(recv, dk, 0, r)
        A.unpack_kv_sum(recv, dv, 1, r)
    t_sum = _time(reduce_pair, args.iters)
    es = recv.element_size()
    read, written = recv.numel() * es, 2 * dk.numel() * es
    # the same rows without replication: every chunk's dk | dv head copied to its own head (usp_copy_rows, 2 launches)
    dk8 = torch.empty(B, Sl, P, D, device=dev, dtype=torch.bfloat16)
    dv8 = torch.empty_like(dk8)

    def copy_pair():
        A.unpack_head_group(recv, dk8.view(B, Sl, P, 1, D), 0)
        A.unpack_head_group(recv, dv8.view(B, Sl, P, 1, D), 1)
    t_copy = _time(copy_pair, args.iters)
    moved_copy = 2 * recv.numel() * es
    print(f"device: {torch.cuda.get_device_name(dev)}; P = {P}, Hkv = {Hkv} (r = {r}), {Sl} rows per chunk, D = {D}, bf16")
    print(f"usp_sum_rows  dk + dv (2 launches): {read / 2**20:7.1f} MiB read + {written / 2**20:6.1f} MiB written in "
          f"{t_sum * 1e6:7.1f} us = {(read + written) / t_sum / 1e12:5.2f} TB/s")
    print(f"usp_copy_rows same rows, no sum   : {moved_copy / 2 / 2**20:7.1f} MiB read + {moved_copy / 2 / 2**20:6.1f} MiB written in "
          f"{t_copy * 1e6:7.1f} us = {moved_copy / t_copy / 1e12:5.2f} TB/s")


if __name__ == "__main__":
    main()
