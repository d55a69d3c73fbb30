"""TEST-ONLY block backend for the CPU orchestration tests of `return_block_mass`: the fp64 oracle backend
(tests/oracle_backend.py) with the one call the block attention mass adds to the seam -- block_mass -- computed by
tests/block_mass_ref.py from the operands and the very lse it is handed, and written as fp32 into `out` (which may be a column
slice of a larger result).  `mass_log` records every call: (q shape, k shape, causal, diag, out shape, out strides, the offset of
`out` inside its storage)."""
import torch

import block_mass_ref as MR
from oracle_backend import OracleBlockBackend


class MassOracleBackend(OracleBlockBackend):
    def __init__(self):
        super().__init__()
        self.mass_log = []

    def block_mass(self, q, k, lse, scale, causal, diag=0, out=None):
        for t in (q, k):
            assert t.dim() == 4 and t.stride(-1) == 1 and t.dtype in (torch.bfloat16, torch.float16) and not t.requires_grad
        assert q.shape[3] in (32, 64, 128) and q.shape[3] == k.shape[3] and q.shape[2] % k.shape[2] == 0
        assert lse.dtype == torch.float32 and tuple(lse.shape) == (q.shape[0], q.shape[2], q.shape[1]) and not lse.requires_grad
        assert lse.stride(-1) == 1 or lse.shape[-1] == 1
        assert isinstance(diag, int) and isinstance(causal, bool)
        nbq, nbk = (q.shape[1] + 127) // 128, (k.shape[1] + 127) // 128
        if out is None:
            out = torch.empty(q.shape[0], q.shape[2], nbq, nbk, dtype=torch.float32)
        assert out.dtype == torch.float32 and tuple(out.shape) == (q.shape[0], q.shape[2], nbq, nbk)
        assert out.stride(-1) == 1 or nbk == 1
        self.mass_log.append((tuple(q.shape), tuple(k.shape), causal, diag, tuple(out.shape), out.stride(), out.storage_offset()))
        out.copy_(MR.mass_ref(q, k, lse, scale, causal, diag).to(torch.float32))
        return out
