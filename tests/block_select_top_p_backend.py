"""TEST-ONLY block backend for the CPU orchestration tests of `block_select=BlockSelectTopP(...)`: the fp64 oracle backend of the
top-k selection (tests/block_select_backend.py) with the one call the top-p selection adds to the seam -- block_select_top_p --
computed by tests/block_select_top_p_ref.py from the fp32 means.  `select_log` records every call; `masks` keeps what each
selection returned."""
import torch

import block_select_top_p_ref as TR
from block_select_backend import SelectOracleBackend


class TopPOracleBackend(SelectOracleBackend):
    def block_select_top_p(self, qbar, kbar, top_p, scale, causal, keep_first=0, keep_local=1, share_group=False, row_block0=0):
        for t in (qbar, kbar):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 4
        assert qbar.shape[0] == kbar.shape[0] and qbar.shape[3] == kbar.shape[3] and qbar.shape[2] % kbar.shape[2] == 0
        assert isinstance(top_p, float) and 0 < top_p <= 1 and isinstance(share_group, bool)
        assert all(isinstance(x, int) and x >= 0 for x in (keep_first, keep_local, row_block0))
        self.select_log.append(("select_top_p", tuple(qbar.shape), tuple(kbar.shape), int(row_block0), bool(causal), share_group))
        mask = TR.select_from_means(qbar, kbar, top_p, scale, bool(causal), keep_first, keep_local, share_group, row_block0)
        self.masks.append(mask)
        return mask
