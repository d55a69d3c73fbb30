"""fp64 restatements of the flash kernels WITH the roundings a 16-bit kernel performs: the "honest" models the input
families of the parity tests are tuned against (a case is fair when the honest model stays inside half of the stated
bound), and the mutants those families must catch.  Plain numpy; shared by tests/test_gpu_row64.py,
tests/test_range_cpu.py and tests/test_gpu_range.py."""
import numpy as np

from golden_util import round_to

LOG2E = 1.4426950408889634
TILE = 64
K_THR = 8.0                                   # the forwards' deferred-max rule: usp_flash_fwd_body.inc / usp_flash_fwd64.hip `kThr`
MAX16 = {"bfloat16": float(np.float32(3.3895313892515355e38)), "float16": 65504.0}
MIN_NORMAL16 = {"bfloat16": 2.0 ** -126, "float16": 2.0 ** -14}


def bwd_16bit_model(do, q, k, v, o16, lse, scale, causal, dt, prescale_k, softcap=None):
    """fp64 restatement of the block backward WITH the two roundings every 16-bit flash backward performs: P is rounded
    to the 16-bit type before dV = P^T dO (and dS is formed from that rounded P), dS is rounded before dQ = dS K and
    dK = dS^T Q.  `prescale_k`: also round K * scale * log2(e) to the 16-bit type, as the 64-row dK/dV kernel did once per item until
    tests/test_gpu_range.py (a mutant now: tests/test_range_cpu.py).  `softcap`: scores capped to cap * tanh(S / cap) before
    the mask, dS times 1 - tanh^2 (include/usp_hip.h USP_ATTN_SOFTCAP)."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    g = Hq // Hkv
    kk, vv = np.repeat(k, g, axis=2).astype(np.float64), np.repeat(v, g, axis=2).astype(np.float64)
    qd, dod = q.astype(np.float64), do.astype(np.float64)
    log2e = 1.4426950408889634
    if prescale_k:
        k2 = round_to((kk * (scale * log2e)).astype(np.float32), dt).astype(np.float64)
        s2 = np.einsum("bthd,bshd->bhts", qd, k2, optimize=True)                 # exponent, base 2
    else:
        s2 = np.einsum("bthd,bshd->bhts", qd, kk, optimize=True) * (scale * log2e)
    dcap = 1.0
    if softcap:
        tanh = np.tanh(s2 / (log2e * softcap))
        s2, dcap = softcap * log2e * tanh, 1.0 - tanh * tanh
    if causal:
        row, col = np.arange(Sq)[:, None], np.arange(Sk)[None, :]
        s2 = np.where(col > row + Sk - Sq, -np.inf, s2)
    lse_safe = np.where(np.isfinite(lse), lse, 0.0)
    p = np.where(np.isfinite(lse)[..., None], np.exp2(s2 - lse_safe[..., None] * log2e), 0.0)
    p16 = round_to(p.astype(np.float32), dt).astype(np.float64)
    dv = np.einsum("bhts,bthd->bshd", p16, dod, optimize=True).reshape(B, Sk, Hkv, g, D).sum(3)
    dp = np.einsum("bthd,bshd->bhts", dod, vv, optimize=True)
    delta = np.einsum("bthd,bthd->bht", dod, o16.astype(np.float64))
    ds16 = round_to((p16 * (dp - delta[..., None]) * dcap).astype(np.float32), dt).astype(np.float64)
    dq = np.einsum("bhts,bshd->bthd", ds16, kk, optimize=True) * scale
    dk = (np.einsum("bhts,bthd->bshd", ds16, qd, optimize=True) * scale).reshape(B, Sk, Hkv, g, D).sum(3)
    return dq, dk, dv


def fwd_16bit_model(q, k, v, scale, causal, dt, raise_max=True, flush_subnormal=False, softcap=None):
    """fp64 restatement of the tiled forward with P rounded to the 16-bit type before P V: 64-key tiles, a reference max
    per row that is raised only when the row's running max grew by more than 2^K_THR (the kernels' deferred-max rule;
    their decision is wave-uniform, so they raise at least as often: P <= 2^K_THR either way), l summed from the
    unrounded P.  -> (out, lse (nat), largest P / 2^reference seen).
    Mutants: `raise_max=False` keeps the first tile's max for ever and clamps P to the 16-bit type's range (what a
    pack does to an overflowing exponential); `flush_subnormal=True` drops every P below the type's smallest normal."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    g = Hq // Hkv
    kk, vv = np.repeat(k, g, axis=2).astype(np.float64), np.repeat(v, g, axis=2).astype(np.float64)
    s = np.einsum("bthd,bshd->bhts", q.astype(np.float64), kk, optimize=True) * scale
    if softcap:
        s = softcap * np.tanh(s / softcap)
    s2 = s * LOG2E
    if causal:
        row, col = np.arange(Sq)[:, None], np.arange(Sk)[None, :]
        s2 = np.where(col > row + Sk - Sq, -np.inf, s2)
    m_ref = np.full((B, Hq, Sq), -np.inf)
    l = np.zeros((B, Hq, Sq))
    acc = np.zeros((B, Hq, Sq, D))
    p_max = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for t0 in range(0, Sk, TILE):
            st = s2[..., t0:t0 + TILE]
            new = np.maximum(m_ref, st.max(-1))
            first = ~np.isfinite(m_ref)
            if raise_max:
                m_new = np.where(first | (new - m_ref > K_THR), new, m_ref)
            else:
                m_new = np.where(first, new, m_ref)
            use = np.where(np.isfinite(m_new), m_new, 0.0)
            alpha = np.where(first, 0.0, np.exp2(np.where(first, 0.0, m_ref) - use))
            p = np.exp2(st - use[..., None])
            p_max = max(p_max, float(p.max()))
            p16 = round_to(np.minimum(p, MAX16[dt]).astype(np.float32), dt).astype(np.float64)
            if flush_subnormal:
                p16 = np.where(p16 < MIN_NORMAL16[dt], 0.0, p16)
            l = l * alpha + np.minimum(p, 3.0e38).sum(-1)
            acc = acc * alpha[..., None] + np.einsum("bhts,bshd->bhtd", p16, vv[:, t0:t0 + TILE], optimize=True)
            m_ref = m_new
        out = np.where(l[..., None] > 0, acc / np.where(l > 0, l, 1.0)[..., None], 0.0).transpose(0, 2, 1, 3)
        lse = np.where(l > 0, (np.where(np.isfinite(m_ref), m_ref, 0.0) + np.log2(np.where(l > 0, l, 1.0))) / LOG2E, -np.inf)
    return out, lse, p_max
