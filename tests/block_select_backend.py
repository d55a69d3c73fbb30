"""TEST-ONLY block backend for the CPU orchestration tests of `block_select=`: the fp64 oracle backend that serves `bsp=`
(tests/test_block_mask_cpu.py: BlockOracleBackend, itself over tests/oracle_backend.py) with the two calls the selection adds to
the seam -- block_means and block_select -- computed by tests/block_select_ref.py.  The means leave as fp32, as the kernel's do
(they travel through the ring's all-gather in that type); the scores and the selection are fp64.  `select_log` records every
call; `masks` keeps what each block_select returned."""
import torch

import block_select_ref as SR
from test_block_mask_cpu import BlockOracleBackend


class SelectOracleBackend(BlockOracleBackend):
    def __init__(self):
        super().__init__()
        self.select_log, self.masks = [], []

    def block_means(self, x):
        assert x.dim() == 4 and x.stride(-1) == 1 and x.dtype in (torch.bfloat16, torch.float16) and not x.requires_grad
        assert x.shape[3] % 8 == 0 and x.shape[3] <= 128, "usp_block_means: D a multiple of 8 up to 128"
        self.select_log.append(("means", tuple(x.shape)))
        return SR.block_means(x).to(torch.float32)

    def block_select(self, qbar, kbar, top_k, scale, causal, keep_first=0, keep_local=1, row_block0=0):
        for t in (qbar, kbar):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 4
        assert qbar.shape[0] == kbar.shape[0] and qbar.shape[3] == kbar.shape[3] and qbar.shape[2] % kbar.shape[2] == 0
        assert all(isinstance(x, int) and x >= 0 for x in (top_k, keep_first, keep_local, row_block0))
        self.select_log.append(("select", tuple(qbar.shape), tuple(kbar.shape), int(row_block0), bool(causal)))
        mask = SR.select_from_scores(SR.scores(qbar, kbar, scale), top_k, bool(causal), keep_first, keep_local, row_block0)
        self.masks.append(mask)
        return mask
