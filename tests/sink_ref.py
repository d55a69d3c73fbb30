"""Exact attention in fp64 with attention sinks (include/usp_hip.h: usp_flash_fwd_sink / usp_sink_bwd), dense and small: the truth
the sink tests hold the block kernels, the rings and the layers against.  Built on tests/alibi_ref.py (scores, mask and the block
backward from a given lse) and so on tests/shift_ref.py's `visible`; tests/test_sink_cpu.py pins it to torch autograd of the
written-out formula (a sink column appended to the scores, softmax, the column dropped).

    lse_i = log(exp(s_h) + sum_j exp(S_ij))      P_ij = exp(S_ij - lse_i)      out_i = sum_j P_ij v_j
    ds_h  = -sum_{b,i} exp(s_h - lse_bhi) * delta_bhi,   delta = rowsum(dout * out)

`sinks` is (Hq,), in score units (not multiplied by the scale); None: no sink (alibi_ref without slopes).  A row without a visible
key gives lse = s_h and out = 0.  dQ, dK, dV are the plain block backward fed this lse.

Also the CPU block backend of the orchestration tests with `sinks=`: SinkOracleBackend.
"""
import torch

import alibi_ref
from oracle_backend import OracleBlockBackend


def ref_fwd(q, k, v, scale, sinks=None, causal=False, window=None, shift=0):
    """-> (out (B,Sq,Hq,D), lse (B,Hq,Sq)), fp64 on q's device."""
    if sinks is None:
        return alibi_ref.ref_fwd(q, k, v, scale, None, causal, window, shift)
    s, _ = alibi_ref._scores(q, k, scale, None, causal, window, shift)
    lse = torch.logaddexp(torch.logsumexp(s, dim=-1), sinks.to(device=q.device, dtype=torch.float64)[None, :, None])
    v64 = v.to(torch.float64).repeat_interleave(q.shape[2] // v.shape[2], dim=2)
    return torch.einsum("bhij,bjhd->bihd", torch.exp(s - lse[..., None]), v64), lse


def sink_terms(sinks, lse, delta):
    """(B,Hq,Sq) fp64: exp(s_h - lse) * delta, 0 where lse = -inf; ds_h = -(their sum over b and i)."""
    lse, delta = lse.to(torch.float64), delta.to(torch.float64)
    fin = torch.isfinite(lse)
    e = torch.exp(sinks.to(device=lse.device, dtype=torch.float64)[None, :, None] - torch.where(fin, lse, torch.zeros_like(lse)))
    return torch.where(fin, e * delta, torch.zeros_like(delta))


def ref_dsinks(sinks, lse, delta):
    """(Hq,) fp64."""
    return -sink_terms(sinks, lse, delta).sum(dim=(0, 2))


def ref_bwd_from(dout, q, k, v, out, lse, scale, sinks=None, causal=False, window=None, shift=0):
    """Block backward given the rows' (sink-including) lse and out -> (dq, dk, dv, dsinks | None), fp64."""
    grads = alibi_ref.ref_bwd_from(dout, q, k, v, out, lse, scale, None, causal, window, shift)
    if sinks is None:
        return grads + (None,)
    delta = (dout.to(torch.float64) * out.to(torch.float64)).sum(-1).transpose(1, 2)
    return grads + (ref_dsinks(sinks, lse, delta),)


def ref_bwd(dout, q, k, v, scale, sinks=None, causal=False, window=None, shift=0, out_dtype=None):
    """Forward + backward of the whole problem -> (out, lse, dq, dk, dv, dsinks), fp64.  `out_dtype`: round `out` to it before
    delta is formed (what a 16-bit kernel's backward reads)."""
    out, lse = ref_fwd(q, k, v, scale, sinks, causal, window, shift)
    o = out if out_dtype is None else out.to(out_dtype)
    return (out, lse) + ref_bwd_from(dout, q, k, v, o, lse, scale, sinks, causal, window, shift)


class SinkOracleBackend(OracleBlockBackend):
    """The oracle block backend with `sinks=` on fwd and `sink_grad`: the sink is applied on host AFTER the wrapped block
    (lse' = logaddexp(lse, s_h), the rows just written scaled by exp(lse - lse')), which is what the kernels' epilogue does.
    Cooperative (`super().fwd`), so it also sits in front of an oracle that takes `shift`.  Logs every forward launch in
    `sink_log`: (first row of the launch in the rank's lse, rows, carried a sink, merge_in)."""

    def __init__(self):
        super().__init__()
        self.sink_log = []

    def fwd(self, q, k, v, softmax_scale, causal, lse, out=None, acc=None, merge_in=False, final_begin=0, final_end=None,
            sinks=None, **kw):
        super().fwd(q, k, v, softmax_scale, causal, lse, out, acc, merge_in, final_begin, final_end, **kw)
        Sq = q.shape[1]
        row0 = lse.storage_offset() % lse.stride(1) if lse.stride(1) >= Sq else 0
        self.sink_log.append((row0, Sq, sinks is not None, bool(merge_in)))
        if sinks is None:
            return
        assert not merge_in, "the sink belongs to the launch that opens the rows' state"
        assert tuple(sinks.shape) == (q.shape[2],), (tuple(sinks.shape), q.shape[2])
        old = lse.to(torch.float64)
        new = torch.logaddexp(old, sinks.detach().to(torch.float64)[None, :, None])
        w = torch.exp(old - new).transpose(1, 2)[..., None]                    # (B,Sq,Hq,1); 0 for an empty row
        lse.copy_(new)
        fe = Sq if final_end is None else final_end
        for dst, rows in ((out, slice(final_begin, fe)), (acc, slice(0, final_begin)), (acc, slice(fe, Sq))):
            if dst is not None and rows.stop > rows.start:
                dst[:, rows].copy_(dst[:, rows].to(torch.float64) * w[:, rows])

    def sink_grad(self, sinks, lse, delta, out=None, accum=False):
        g = ref_dsinks(sinks.detach(), lse, delta).to(torch.float32)
        if out is None:
            return g
        out.copy_(out + g if accum else g)
        return out
