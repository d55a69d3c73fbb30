"""ctypes binding of libusp_hip.so (C ABI: include/usp_hip.h).

This is the ONLY device backend of the package.  There is no CPU or eager-PyTorch fallback: if the
library is missing, or a tensor is not a CUDA(ROCm) tensor, the call raises.  PyTorch is used for
device memory and streams only; every kernel runs on ``torch.cuda.current_stream()``.
"""
from __future__ import annotations

import ctypes
import math
import os
import struct
import threading
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libusp_hip.so")
_lib = None

USP_BF16, USP_FP16 = 0, 1
USP_LAUNCH_INTERLEAVE = 1      # include/usp_hip.h: launch so that collectives on other streams can slip in
USP_ATTN_WINDOW = 2            # the window_left / window_right fields are valid
USP_FORCE_ROW64 = 4            # ABI v6: the call must be served by the one-wave-per-SIMD (64-row) kernel family ...
USP_FORCE_WAVE32 = 8           # ... or by the two-waves-per-SIMD (32 rows per wave) family
USP_BWD_SKIP_DQ = 16           # usp_flash_bwd: only the dK/dV launch ...
USP_BWD_SKIP_DKDV = 32         # ... only the dQ launch
USP_ATTN_SOFTCAP = 64          # the softcap field is valid: scores are capped to softcap * tanh(S / softcap)
USP_ATTN_SHIFT = 128           # the mask_shift field is valid: (Sk - Sq) + mask_shift places the diagonal of every mask bound
USP_ATTN_ALIBI = 256           # feature bit of usp_attn_features(): usp_flash_fwd_alibi / usp_flash_bwd_alibi exist (not an args flag)
USP_ATTN_DROPOUT = 512         # feature bit of usp_attn_features(): usp_flash_fwd_dropout / usp_flash_bwd_dropout exist (not an args flag)
USP_ATTN_SINK = 1024           # feature bit of usp_attn_features(): usp_flash_fwd_sink / usp_sink_bwd exist (not an args flag)
USP_ATTN_DOC = 2048            # feature bit of usp_attn_features(): usp_flash_fwd_doc / usp_flash_bwd_doc exist (not an args flag)
USP_ATTN_SPAN = 4096           # feature bit of usp_attn_features(): usp_flash_fwd_span / usp_flash_bwd_span exist (not an args flag)
USP_ATTN_BLOCK_MASK = 8192     # feature bit of usp_attn_features(): usp_block_list_bytes / usp_flash_fwd_bsp / usp_flash_bwd_bsp exist (not an args flag)
USP_ATTN_MAX_LOGIT = 16384     # feature bit of usp_attn_features(): usp_flash_fwd_maxlogit / usp_row_max_reduce exist (not an args flag)
USP_ATTN_BLOCK_SELECT = 32768  # feature bit of usp_attn_features(): usp_block_means / usp_block_select exist (not an args flag)
USP_DKDV_KEYS256 = 65536       # usp_flash_bwd: 256-key items for the 64-row family's dK/dV launch (one wave does all four products) ...
USP_DKDV_KEYS128 = 131072      # ... or its 128-key items (two waves share a 64-key slice); neither: the library picks per launch
USP_ATTN_BLOCK_SELECT_TOP_P = 65536  # feature bit of usp_attn_features(): usp_block_select_top_p exists (not an args flag)
USP_ATTN_BLOCK_MASS = 131072   # feature bit of usp_attn_features(): usp_block_attn_mass exists (not an args flag)
BLOCK_SELECT_MAX_BLOCKS = 8192 # key blocks of one usp_block_select call (include/usp_hip.h: USP_BLOCK_SELECT_MAX_BLOCKS)
BLOCK_MASK_SIZE = 128          # rows and keys of one block of a block mask (include/usp_hip.h: USP_BLOCK_MASK_SIZE)
ABI_VERSION = 7
# usp_last_launch_kinds(): bit -> kernel (include/usp_hip.h, USP_KIND_*)
KINDS = {1: "fwd_row64", 2: "fwd_wave8", 4: "fwd_wave4", 8: "fwd_split_merge", 16: "dkdv_row64", 32: "dkdv_wave8",
         64: "dq_row64", 128: "dq_wave8", 256: "reduce_heads", 512: "reduce_cuts"}
_FAMILY_FLAG = {None: 0, "auto": 0, "row64": USP_FORCE_ROW64, "wave32": USP_FORCE_WAVE32}
# In-process default of the `family` argument of flash_fwd / flash_bwd (tests, A/B runs: bench.py times both families
# on the same box).  "auto": the library decides per launch.
_FAMILY_DEFAULT = "auto"


def set_kernel_family(family) -> str:
    """Default kernel family of dense flash launches issued through this binding: "auto" | "row64" | "wave32";
    returns the previous setting.  Per call the `family` argument overrides it."""
    global _FAMILY_DEFAULT
    if family not in _FAMILY_FLAG:
        raise ValueError(f"kernel family must be one of {sorted(k for k in _FAMILY_FLAG if k)}, got {family!r}")
    prev, _FAMILY_DEFAULT = _FAMILY_DEFAULT, (family or "auto")
    return prev


def _family_flag(family) -> int:
    if family is None:
        family = _FAMILY_DEFAULT
    try:
        return _FAMILY_FLAG[family]
    except KeyError:
        raise ValueError(f"kernel family must be one of {sorted(k for k in _FAMILY_FLAG if k)}, got {family!r}") from None


_DKDV_KEYS_FLAG = {0: 0, None: 0, 128: USP_DKDV_KEYS128, 256: USP_DKDV_KEYS256}
USP_KIND_DKDV_KEYS256 = 1024   # beside "dkdv_row64": the 256-key-item kernel ran (not a kernel of its own: not in KINDS)


def last_dkdv_item_keys() -> int:
    """Keys per work item of the 64-row dK/dV kernel the calling thread's last flash_bwd launched: 128 | 256; 0 if it launched none."""
    m = load().usp_last_launch_kinds()
    return 0 if not m & 16 else (256 if m & USP_KIND_DKDV_KEYS256 else 128)


def last_launch_kinds() -> tuple:
    """Names of the kernels the calling thread's last flash_fwd / flash_bwd launched (usp_last_launch_kinds)."""
    m = load().usp_last_launch_kinds()
    return tuple(name for bit, name in KINDS.items() if m & bit)


class UspTensor(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("stride_b", ctypes.c_int64),
                ("stride_s", ctypes.c_int64), ("stride_h", ctypes.c_int64)]


class UspFwdArgs(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("Sq", ctypes.c_int32),
                ("Sk", ctypes.c_int32), ("Hq", ctypes.c_int32), ("Hkv", ctypes.c_int32),
                ("D", ctypes.c_int32), ("causal", ctypes.c_int32),
                ("softmax_scale", ctypes.c_float), ("mask_shift", ctypes.c_int32),
                ("q", UspTensor), ("k", UspTensor), ("v", UspTensor),
                ("out", UspTensor), ("acc", UspTensor),
                ("lse", ctypes.c_void_p), ("lse_stride_b", ctypes.c_int64),
                ("lse_stride_h", ctypes.c_int64),
                ("merge_in", ctypes.c_int32), ("final_begin", ctypes.c_int32),
                ("final_end", ctypes.c_int32),
                ("seq_q", ctypes.c_void_p), ("seq_k", ctypes.c_void_p), ("sched", ctypes.c_void_p),
                ("flags", ctypes.c_int32), ("k_splits", ctypes.c_int32), ("workspace", ctypes.c_void_p),
                ("window_left", ctypes.c_int32), ("window_right", ctypes.c_int32),
                ("softcap", ctypes.c_float)]


class UspBwdArgs(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("Sq", ctypes.c_int32),
                ("Sk", ctypes.c_int32), ("Hq", ctypes.c_int32), ("Hkv", ctypes.c_int32),
                ("D", ctypes.c_int32), ("causal", ctypes.c_int32),
                ("softmax_scale", ctypes.c_float), ("mask_shift", ctypes.c_int32),
                ("dout", UspTensor), ("q", UspTensor), ("k", UspTensor), ("v", UspTensor),
                ("lse", ctypes.c_void_p), ("delta", ctypes.c_void_p),
                ("lse_stride_b", ctypes.c_int64), ("lse_stride_h", ctypes.c_int64),
                ("delta_stride_b", ctypes.c_int64), ("delta_stride_h", ctypes.c_int64),
                ("dq", UspTensor), ("dk", UspTensor), ("dv", UspTensor),
                ("accum_dq", ctypes.c_int32), ("accum_dk", ctypes.c_int32),
                ("accum_dv", ctypes.c_int32),
                ("dq16", UspTensor), ("dk16", UspTensor), ("dv16", UspTensor),
                ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
                ("seq_q", ctypes.c_void_p), ("seq_k", ctypes.c_void_p), ("total_k", ctypes.c_int64),
                ("sched", ctypes.c_void_p), ("flags", ctypes.c_int32),
                ("dq_splits", ctypes.c_int32), ("dkdv_splits", ctypes.c_int32),
                ("window_left", ctypes.c_int32), ("window_right", ctypes.c_int32),
                ("dkdv_heads", ctypes.c_int32), ("softcap", ctypes.c_float)]


EXPORTS = ("usp_flash_fwd", "usp_flash_fwd_workspace_bytes", "usp_flash_bwd", "usp_flash_bwd_workspace_bytes", "usp_bwd_delta", "usp_lse_merge", "usp_copy_rows",
           "usp_sum_rows", "usp_cast_from_f32", "usp_add_f32", "usp_abi_version", "usp_strerror", "usp_last_launch_kinds", "usp_mfma_probe",
           "usp_attn_features", "usp_flash_fwd_alibi", "usp_flash_bwd_alibi", "usp_flash_fwd_dropout", "usp_flash_bwd_dropout",
           "usp_flash_fwd_sink", "usp_sink_bwd", "usp_flash_fwd_doc", "usp_flash_bwd_doc", "usp_flash_fwd_span", "usp_flash_bwd_span",
           "usp_block_list_bytes", "usp_block_lists_build", "usp_flash_fwd_bsp", "usp_flash_bwd_bsp",
           "usp_flash_fwd_maxlogit", "usp_row_max_reduce", "usp_block_means", "usp_block_select",
           "usp_block_select_top_p", "usp_block_attn_mass")
# The entry points of ALiBi, dropout, the sinks, the document mask and the spans are the only exports load() does not insist on: they are
# looked up and prototyped on first use (_feature_entry), behind their feature bit, so a library built before them still loads
# and serves everything else.
ALIBI_EXPORTS = ("usp_flash_fwd_alibi", "usp_flash_bwd_alibi")
DROPOUT_EXPORTS = ("usp_flash_fwd_dropout", "usp_flash_bwd_dropout")
SINK_EXPORTS = ("usp_flash_fwd_sink", "usp_sink_bwd")
DOC_EXPORTS = ("usp_flash_fwd_doc", "usp_flash_bwd_doc")
SPAN_EXPORTS = ("usp_flash_fwd_span", "usp_flash_bwd_span")
BSP_EXPORTS = ("usp_block_list_bytes", "usp_block_lists_build", "usp_flash_fwd_bsp", "usp_flash_bwd_bsp")
MAXL_EXPORTS = ("usp_flash_fwd_maxlogit", "usp_row_max_reduce")
SELECT_EXPORTS = ("usp_block_means", "usp_block_select")
SELECT_TOP_P_EXPORTS = ("usp_block_select_top_p",)
MASS_EXPORTS = ("usp_block_attn_mass",)


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Load libusp_hip.so (once).  Raises RuntimeError, loudly, when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"libusp_hip.so not found at {_LIB_PATH}: the HIP extension is not built. Run "
            f"`python -c 'import __graft_entry__ as g; g.build()'` or "
            f"`make -C long-context-attention_amd/csrc`. There is no CPU fallback.")
    L = ctypes.CDLL(_LIB_PATH)
    for name in EXPORTS:
        if name not in ALIBI_EXPORTS + DROPOUT_EXPORTS + SINK_EXPORTS + DOC_EXPORTS + SPAN_EXPORTS + BSP_EXPORTS + MAXL_EXPORTS + SELECT_EXPORTS + SELECT_TOP_P_EXPORTS + MASS_EXPORTS and not hasattr(L, name):
            raise RuntimeError(f"{_LIB_PATH} does not export {name} (stale build?)")
    L.usp_strerror.restype = ctypes.c_char_p
    L.usp_abi_version.restype = ctypes.c_int
    L.usp_last_launch_kinds.restype = ctypes.c_int
    L.usp_last_launch_kinds.argtypes = []
    L.usp_attn_features.restype = ctypes.c_int
    L.usp_attn_features.argtypes = []
    if L.usp_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libusp_hip.so ABI {L.usp_abi_version()} != binding ABI {ABI_VERSION}")
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    L.usp_flash_fwd.argtypes = [ctypes.POINTER(UspFwdArgs), vp]
    L.usp_flash_bwd.argtypes = [ctypes.POINTER(UspBwdArgs), vp]
    L.usp_flash_fwd_workspace_bytes.argtypes = [ctypes.POINTER(UspFwdArgs), i32]
    L.usp_flash_fwd_workspace_bytes.restype = ctypes.c_int64
    L.usp_flash_bwd_workspace_bytes.argtypes = [ctypes.POINTER(UspBwdArgs)]
    L.usp_flash_bwd_workspace_bytes.restype = ctypes.c_int64
    L.usp_bwd_delta.argtypes = [i32, i32, i32, i32, i32, ctypes.POINTER(UspTensor),
                                ctypes.POINTER(UspTensor), vp, i64, i64, vp]
    L.usp_lse_merge.argtypes = [i32, i32, i32, i32, i32, ctypes.POINTER(UspTensor), vp, i64, i64,
                                ctypes.POINTER(UspTensor), vp, i64, i64, i32, vp]
    L.usp_copy_rows.argtypes = [vp, vp] + [i64] * 13 + [vp]
    L.usp_sum_rows.argtypes = [i32, vp, vp, i64, i32] + [i64] * 10 + [vp]
    L.usp_cast_from_f32.argtypes = [i32, vp, i64, vp, i64, i64, i64, vp]
    L.usp_add_f32.argtypes = [vp, i64, vp, i64, vp, i64, i64, i64, vp]
    L.usp_mfma_probe.argtypes = [vp, i64, i32, i32, vp, vp, vp]
    L.usp_mfma_probe.restype = ctypes.c_int
    for name in ("usp_flash_fwd", "usp_flash_bwd", "usp_bwd_delta", "usp_lse_merge", "usp_copy_rows", "usp_sum_rows",
                 "usp_cast_from_f32", "usp_add_f32"):
        getattr(L, name).restype = ctypes.c_int
    _lib = L
    return L


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {load().usp_strerror(rc).decode()} (code {rc})")


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dtype_code(dtype: torch.dtype) -> int:
    if dtype == torch.bfloat16:
        return USP_BF16
    if dtype == torch.float16:
        return USP_FP16
    raise TypeError(f"libusp_hip supports bfloat16 / float16 inputs, got {dtype}")


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "libusp_hip kernels need ROCm device tensors (got a CPU tensor); there is no CPU "
                "fallback in this package")


def _t4(t: Optional[torch.Tensor]) -> UspTensor:
    """(B,S,H,D) view with unit dim stride -> usp_tensor."""
    if t is None:
        return UspTensor(None, 0, 0, 0)
    assert t.dim() == 4, t.shape
    if t.stride(3) != 1:
        raise ValueError("last (head_dim) stride must be 1")
    return UspTensor(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))


def _lse3(t: torch.Tensor):
    """(B,H,S) fp32 with unit seq stride -> (ptr, stride_b, stride_h)."""
    assert t.dim() == 3 and t.dtype == torch.float32
    if t.shape[2] > 1 and t.stride(2) != 1:
        raise ValueError("lse/delta must have unit stride along the sequence")
    return ctypes.c_void_p(t.data_ptr()), t.stride(0), t.stride(1)


_FWD_WS = {}


def _parse_ksplit(raw) -> object:
    """USP_FWD_KSPLIT -> "auto" | 0 | n in 2..8.  Anything else counts as off, with one warning (a typo in an
    environment variable must not raise on every launch)."""
    raw = (raw or "auto").strip().lower()
    if raw in ("auto", "0"):
        return "auto" if raw == "auto" else 0
    try:
        n = int(raw)
    except ValueError:
        import warnings
        warnings.warn(f"USP_FWD_KSPLIT={raw!r} is neither 'auto', 0 nor an integer: the K split stays off")
        return 0
    return 0 if n < 2 else min(n, 8)


# Read ONCE, at import (a launch does not touch os.environ); set_fwd_ksplit changes it in-process (tests, A/B runs).
_KSPLIT_MODE = _parse_ksplit(os.environ.get("USP_FWD_KSPLIT"))


def set_fwd_ksplit(mode) -> object:
    """Set the K-split policy of dense forward launches ("auto" | 0 | n); returns the previous one."""
    global _KSPLIT_MODE
    prev, _KSPLIT_MODE = _KSPLIT_MODE, _parse_ksplit(str(mode))
    return prev


def fwd_k_splits(B: int, Sq: int, Hq: int, causal: bool) -> int:
    """How many work items a dense forward launch cuts every query tile's keys into (usp_fwd_args.k_splits).  A causal
    launch with fewer than two 256-row items per CU lasts as long as its heaviest item; cutting every item's keys into n
    equal runs (partials + one HBM-bound merge launch) fills the part.  Measured natively on MI355X (`kbench ksplit`,
    profiles/r02_kbench_ksplit*.log: B1 S16384 D128 causal, 2 heads 557 -> 936 TFLOP/s at n = 4, 4 heads 798 -> 1070 at
    n = 2, merge launch included; 8 heads fill the part and gain nothing) and, through this binding, by
    tests/test_gpu_parity.py::test_forward_k_split_through_the_binding.  Policy (USP_FWD_KSPLIT, read at import):
        auto (default)  causal launches of >= 4096 rows with fewer than two 256-row items per CU: n = 2 from 256 items
                        up, 4 below (the measured optima);
        n               n cuts (2..8) for every causal launch with fewer than two 256-row items per CU;
        0               off."""
    mode = _KSPLIT_MODE
    if mode == 0 or not causal:
        return 0
    items = B * Hq * ((Sq + 255) // 256)
    if items >= 512:
        return 0
    if mode == "auto":
        return 0 if Sq < 4096 else (2 if items >= 256 else 4)
    return mode


_BWD_SPLIT_MODE = _parse_ksplit(os.environ.get("USP_BWD_SPLIT"))      # same grammar as USP_FWD_KSPLIT


def set_bwd_split(mode) -> object:
    """Set the cut policy of dense backward launches ("auto" | 0 | n); returns the previous one."""
    global _BWD_SPLIT_MODE
    prev, _BWD_SPLIT_MODE = _BWD_SPLIT_MODE, _parse_ksplit(str(mode))
    return prev


def bwd_splits(B: int, Sq: int, Sk: int, Hq: int, causal: bool):
    """(dq_splits, dkdv_splits) of a dense backward call (usp_bwd_args, ABI v5): the dQ launch has B*Hq*ceil(Sq/256) work
    items and the dK/dV launch B*Hq*ceil(Sk/128) (one per query head and key block); with fewer than two per CU a
    causal launch lasts as long as its heaviest item, with fewer than one per CU any launch leaves CUs idle -- such items
    are cut (dQ along the keys, dK/dV along the query rows; partials + one reduce launch).  Measured on MI355X
    (`kbench bwd` with USP_KBENCH_BWD_SPLITS, profiles/r03_kbench_bwd_cuts.log), B1 S16384 D128 causal: 2 query heads
    394 -> 737 TFLOP/s at (4, 2), 4 heads 688 -> 808 at (2, 1); 8 heads (827) and 4 heads at S32768 (847) fill the part
    and lose 3-6 % to any cut.  Policy (USP_BWD_SPLIT = auto | 0 | n, read at import): auto = per launch, n = 2 from
    256 items up (causal only), 4 below; rows >= 4096 only."""
    mode = _BWD_SPLIT_MODE
    if mode == 0:
        return 0, 0

    def cuts(items, rows):
        if rows < 4096 or items >= 512 or (items >= 256 and not causal):
            return 0
        if mode != "auto":
            return mode
        return 2 if items >= 256 else 4
    return cuts(B * Hq * ((Sq + 255) // 256), Sq), cuts(B * Hq * ((Sk + 127) // 128), Sk)


_TLS = threading.local()      # per-thread cache of filled argument blocks (the autograd thread launches too)
_ARGS_CACHE_MAX = 64


def _strides(t):
    return None if t is None else t.stride()


def _window(window):
    """flash-attn's `window_size` -> (left, right) ints, or None for no window ((-1, -1) / None)."""
    if window is None:
        return None
    wl, wr = int(window[0]), int(window[1])
    return None if (wl < 0 and wr < 0) else (wl, wr)


def softcap_value(softcap) -> Optional[float]:
    """flash-attn's `softcap` -> the cap as a float, or None when it is off (None / 0).  flash-attn silently ignores a
    negative value; this package fails loudly instead: a negative, NaN or infinite cap raises ValueError.  (Pure
    argument check: the CPU orchestration tests call it without a library.)"""
    if softcap is None:
        return None
    cap = float(softcap)
    if cap == 0.0:
        return None
    if not (math.isfinite(cap) and cap > 0.0):
        raise ValueError(f"softcap must be a finite number > 0 (0 / None = off), got {softcap!r}")
    return cap


def _set_softcap(a, cap: Optional[float]):
    """Set USP_ATTN_SOFTCAP + the field on an argument block; a library that does not report the bit
    (usp_attn_features) would ignore it silently, so it is refused here."""
    if cap is None:
        return
    L = load()
    if not (hasattr(L, "usp_attn_features") and L.usp_attn_features() & USP_ATTN_SOFTCAP):
        raise NotImplementedError(f"{_LIB_PATH} does not serve softcap (USP_ATTN_SOFTCAP): rebuild it")
    a.flags |= USP_ATTN_SOFTCAP
    a.softcap = cap


def alibi_value(alibi_slopes, B: int, Hq: int, device):
    """flash-attn's `alibi_slopes` -> (contiguous fp32 device tensor, batch stride in elements) as usp_flash_fwd_alibi takes
    them, or None when it is off.  Shape (Hq,) (stride 0: one vector for the whole batch) or (B, Hq); any other shape, a dtype
    other than float32 (flash-attn requires fp32 too) or a tensor on another device raises ValueError.  (Pure argument check:
    the CPU orchestration tests call it without a library.)"""
    if alibi_slopes is None:
        return None
    if not isinstance(alibi_slopes, torch.Tensor):
        raise ValueError(f"alibi_slopes must be a torch.Tensor, got {type(alibi_slopes).__name__}")
    if alibi_slopes.dtype != torch.float32:
        raise ValueError(f"alibi_slopes must be float32, got {alibi_slopes.dtype}")
    if tuple(alibi_slopes.shape) not in ((Hq,), (B, Hq)):
        raise ValueError(f"alibi_slopes must have shape ({Hq},) or ({B}, {Hq}), got {tuple(alibi_slopes.shape)}")
    if alibi_slopes.device != torch.device(device):
        raise ValueError(f"alibi_slopes is on {alibi_slopes.device}, the operands on {device}")
    t = alibi_slopes.contiguous()
    return t, (Hq if t.dim() == 2 else 0)


def dropout_value(dropout_p) -> Optional[float]:
    """flash-attn's `dropout_p` -> the drop probability as a float, or None when it is off (None / 0).  NaN, a negative value
    or one >= 1 raises ValueError.  (Pure argument check: the CPU orchestration tests call it without a library.)"""
    if dropout_p is None:
        return None
    p = float(dropout_p)
    if p == 0.0:
        return None
    if not (0.0 < p < 1.0):
        raise ValueError(f"dropout_p must lie in [0, 1) (0 / None = off), got {dropout_p!r}")
    return p


def dropout_threshold(p: float) -> int:
    """The keep threshold min(256, max(1, lrintf((1 - p) * 256))) of include/usp_hip.h, formed in float32 as the library does."""
    f32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]
    return min(256, max(1, round(f32(f32(1.0 - f32(p)) * 256.0))))      # (round: half to even, like lrintf)


def dropout_args(dropout):
    """A block call's `dropout` keyword -> (p, seed, row0, key0, head0) as usp_flash_fwd_dropout takes them, or None when it is
    off (None, or p = 0).  `dropout` = (p, seed, row0, key0, head0): drop probability, 64-bit seed and the global position of
    the launch's row 0, key 0 and query head 0 -- the mask is a function of global (batch, head, row, key) alone
    (include/usp_hip.h).  A p whose keep threshold is 256 (p < 1/512) drops nothing: it is off too, and like the C entry points
    this function then does not look at the rest.  Otherwise negative numbers and a seed outside 64 bits raise ValueError."""
    if dropout is None:
        return None
    p, seed, row0, key0, head0 = dropout
    p = dropout_value(p)
    if p is None or dropout_threshold(p) == 256:
        return None
    seed, row0, key0, head0 = int(seed), int(row0), int(key0), int(head0)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"dropout seed must fit 64 unsigned bits, got {seed}")
    if min(row0, key0, head0) < 0 or max(row0, key0, head0) >= 1 << 31:
        raise ValueError(f"dropout offsets (row0, key0, head0) must lie in [0, 2^31), got {(row0, key0, head0)}")
    return p, seed, row0, key0, head0


def sinks_value(sinks, Hq: int, device, dtype=None):
    """A `sinks` argument -> the contiguous fp32 device tensor usp_flash_fwd_sink / usp_sink_bwd take, or None when it is off.
    One learned logit per query head, in score units: shape (Hq,), float32 or the operands' 16-bit type (`dtype`; None: either
    16-bit type), on the operands' device; anything else raises ValueError.  (Pure argument check: the CPU orchestration tests
    call it without a library.)"""
    if sinks is None:
        return None
    if not isinstance(sinks, torch.Tensor):
        raise ValueError(f"sinks must be a torch.Tensor, got {type(sinks).__name__}")
    if tuple(sinks.shape) != (Hq,):
        raise ValueError(f"sinks must have shape ({Hq},): one logit per query head, got {tuple(sinks.shape)}")
    ok = (torch.float32,) + ((torch.bfloat16, torch.float16) if dtype is None else (dtype,))
    if sinks.dtype not in ok:
        raise ValueError(f"sinks must be float32 or the operands' 16-bit type, got {sinks.dtype}")
    if sinks.device != torch.device(device):
        raise ValueError(f"sinks is on {sinks.device}, the operands on {device}")
    return sinks.detach().float().contiguous()


def doc_value(doc, B: int, Sq: int, Sk: int, device):
    """A block call's `doc` keyword -> ((row_lo, batch stride), (key_hi, batch stride)) as usp_flash_fwd_doc / usp_flash_bwd_doc
    take them, or None when it is off.  `doc` = (row_lo, key_hi): contiguous int32 DEVICE tensors of shape (Sq,) or (B, Sq) and
    (Sk,) or (B, Sk) in the launch's own coordinates (include/usp_hip.h; built on the host by ring/doc_blocks.py); either may be
    None where the call does not read it (the forward reads row_lo alone).  Anything else raises ValueError.  (Pure argument
    check: the CPU orchestration tests call it without a library.)"""
    if doc is None:
        return None
    row_lo, key_hi = doc
    if row_lo is None and key_hi is None:
        return None

    def one(t, n, what):
        if t is None:
            return None, 0
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise ValueError(f"doc {what} must be an int32 torch.Tensor")
        if tuple(t.shape) not in ((n,), (B, n)) or not t.is_contiguous():
            raise ValueError(f"doc {what} must be contiguous with shape ({n},) or ({B}, {n}), got {tuple(t.shape)}")
        if t.device != torch.device(device):
            raise ValueError(f"doc {what} is on {t.device}, the operands on {device}")
        return t, (n if t.dim() == 2 else 0)
    return one(row_lo, Sq, "row_lo"), one(key_hi, Sk, "key_hi")


def span_value(span, B: int, Sq: int, Sk: int, device):
    """A block call's `span` keyword -> four (tensor, batch stride) pairs (row_lo, row_hi, key_lo, key_hi) as usp_flash_fwd_span /
    usp_flash_bwd_span take them, or None when it is off.  `span` = (row_lo, row_hi, key_lo, key_hi): contiguous int32 DEVICE
    tensors of shape (Sq,) or (B, Sq) for the row arrays and (Sk,) or (B, Sk) for the key arrays, in the launch's own
    coordinates, the diagonal folded into row_hi (include/usp_hip.h; built on the host by ring/doc_blocks.py); any may be None
    where the call does not read it (the forward reads the row arrays alone).  Anything else raises ValueError.  (Pure argument
    check: the CPU orchestration tests call it without a library.)"""
    if span is None:
        return None
    if len(span) != 4:
        raise ValueError(f"span must be (row_lo, row_hi, key_lo, key_hi), got {len(span)} entries")
    if all(t is None for t in span):
        return None

    def one(t, n, what):
        if t is None:
            return None, 0
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise ValueError(f"span {what} must be an int32 torch.Tensor")
        if tuple(t.shape) not in ((n,), (B, n)) or not t.is_contiguous():
            raise ValueError(f"span {what} must be contiguous with shape ({n},) or ({B}, {n}), got {tuple(t.shape)}")
        if t.device != torch.device(device):
            raise ValueError(f"span {what} is on {t.device}, the operands on {device}")
        return t, (n if t.dim() == 2 else 0)
    return tuple(one(t, n, what) for t, n, what in zip(span, (Sq, Sq, Sk, Sk), ("row_lo", "row_hi", "key_lo", "key_hi")))


def block_mask_value(mask, B: int, Hq: int, S: int, device):
    """A `block_mask` / `bsp` argument -> (mask as a (B, Hq, nb, nb) uint8 view, byte strides of batch, head, row block) as
    usp_flash_fwd_bsp / usp_flash_bwd_bsp take them, or None when it is off.  A torch.bool tensor on the operands' device of shape
    (nb, nb), (Hq, nb, nb) or (B, Hq, nb, nb), nb = ceil(S / BLOCK_MASK_SIZE); missing dimensions become stride 0 (no copy).  Any
    strides are taken as they are while the last dimension has stride 1; otherwise the value is made contiguous once.  Anything
    else raises ValueError.  Nothing here reads the mask's values.  (Pure argument check: the CPU orchestration tests call it
    without a library.)"""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
        raise ValueError(f"block_mask must be a torch.bool tensor, got {getattr(mask, 'dtype', type(mask).__name__)}")
    nb = (S + BLOCK_MASK_SIZE - 1) // BLOCK_MASK_SIZE
    if tuple(mask.shape) not in ((nb, nb), (Hq, nb, nb), (B, Hq, nb, nb)):
        raise ValueError(f"block_mask must have shape ({nb}, {nb}), ({Hq}, {nb}, {nb}) or ({B}, {Hq}, {nb}, {nb}) "
                         f"({BLOCK_MASK_SIZE} x {BLOCK_MASK_SIZE} blocks of {S} rows), got {tuple(mask.shape)}")
    if mask.device != torch.device(device):
        raise ValueError(f"block_mask is on {mask.device}, the operands on {device}")
    m = mask.detach()
    if nb > 1 and m.stride(-1) != 1:
        m = m.contiguous()
    m = m.view(torch.uint8)
    sr = m.stride(-2) if nb > 1 else nb
    sh = m.stride(-3) if m.dim() >= 3 else 0
    sb = m.stride(0) if m.dim() == 4 else 0
    return m, sb, sh, sr


def block_list_bytes(B: int, Hq: int, nb: int) -> int:
    """usp_block_list_bytes: the scratch a block-sparse call of nb x nb blocks needs for its lists."""
    return int(_feature_entry("usp_block_list_bytes")(B, Hq, nb, nb))


def block_list_layout(B: int, Hq: int, nb: int) -> dict:
    """Where the lists lie in that scratch, in int32 elements (csrc/usp_host.hpp: BlockLists): family -> (offset of the first
    list, lists per (batch, head), ints per list); every list is [count, entries ...].  "fwd": per 128-row block, 64-key tiles;
    "dq": per pair of row blocks, 4 * tile + the live halves' bits; "dkdv": per 128-key block, 64-row tiles."""
    nqb, lf = (nb + 1) // 2, 2 * nb + 2
    off_q = B * Hq * nb * lf
    return dict(fwd=(0, nb, lf), dq=(off_q, nqb, lf), dkdv=(off_q + B * Hq * nqb * lf, nb, lf), ints=off_q + B * Hq * (nqb + nb) * lf)


def block_lists_build(mask, B: int, Hq: int, S: int, causal: bool, lists, which: int = 7):
    """usp_block_lists_build: the builder launch alone, into `lists` (a contiguous device tensor of block_list_bytes bytes);
    which: 1 forward, 2 dQ, 4 dK/dV lists, any sum."""
    m, sb, sh, sr = block_mask_value(mask, B, Hq, S, lists.device)
    _check(_feature_entry("usp_block_lists_build")(_ptr(m), sb, sh, sr, B, Hq, S, 1 if causal else 0, int(which), _ptr(lists), _stream()),
           "usp_block_lists_build")


def _bsp_call(which: str, a, bsp, lists=None):
    """Issues the flash launch `which` of `a` under the block mask `bsp` (block_mask_value).  `lists`: the scratch of the
    lists (a uint8 / int32 device tensor of block_list_bytes; tests read it back); None: from the caching allocator
    (stream-ordered, no host read)."""
    m, sb, sh, sr = bsp
    nb = (a.Sq + BLOCK_MASK_SIZE - 1) // BLOCK_MASK_SIZE
    need = block_list_bytes(a.B, a.Hq, nb)
    if lists is None:
        lists = torch.empty(need, dtype=torch.uint8, device=m.device)
    elif lists.numel() * lists.element_size() < need or not lists.is_contiguous() or lists.device != m.device:
        raise ValueError(f"bsp_lists must be a contiguous device tensor of at least {need} bytes")
    name = f"usp_flash_{which}_bsp"
    _check(_feature_entry(name)(ctypes.byref(a), _ptr(m), sb, sh, sr, _ptr(lists), _stream()), name)


def block_select_value(top_k, keep_first=0, keep_local=1, causal=False):
    """The checked host integers of a block selection (kernels/features.py: BlockSelect): (top_k, keep_first, keep_local).
    ValueError: a top_k that is no int (a bool is none), a keep_first / keep_local that is none, a negative value, and
    keep_local < 1 under `causal` (no row may be left without its own block).  (Pure argument check.)"""
    for name, x in (("top_k", top_k), ("keep_first", keep_first), ("keep_local", keep_local)):
        if isinstance(x, bool) or not isinstance(x, int):
            raise ValueError(f"block_select: {name} must be an int, got {x!r}")
        if x < 0:
            raise ValueError(f"block_select: {name} must be >= 0, got {x}")
    if causal and keep_local < 1:
        raise ValueError(f"block_select: a causal selection needs keep_local >= 1 (every row keeps its own block), got {keep_local}")
    i32max = (1 << 31) - 1
    return min(top_k, i32max), min(keep_first, i32max), min(keep_local, i32max)


def block_means(x, out=None):
    """usp_block_means: the fp32 means (B, nb, H, D) of the BLOCK_MASK_SIZE-row blocks of a 16-bit (B, S, H, D) tensor with unit
    head-dim stride (16-byte aligned, strides multiples of 8 elements: kernels/attention.py: kernel_operand), D a multiple of 8
    up to 128.  The last block is divided by its own row count.  `out`: a contiguous fp32 (B, nb, H, D) device tensor."""
    _require_cuda(x)
    B, S, H, D = x.shape
    nb = (S + BLOCK_MASK_SIZE - 1) // BLOCK_MASK_SIZE
    if out is None:
        out = torch.empty((B, nb, H, D), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, nb, H, D) or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"block_means: out must be a contiguous fp32 ({B}, {nb}, {H}, {D}) tensor on {x.device}")
    t = _t4(x)
    _check(_feature_entry("usp_block_means")(t.ptr, dtype_code(x.dtype), B, S, H, D, t.stride_b, t.stride_s, t.stride_h, _ptr(out),
                                             _stream()), "usp_block_means")
    return out


def block_select(qbar, kbar, top_k, scale: float, causal: bool, keep_first: int = 0, keep_local: int = 1, row_block0: int = 0,
                 out=None):
    """usp_block_select: the torch.bool mask (B, Hq, nbq, nbk) of the means qbar fp32 (B, nbq, Hq, D) and kbar fp32
    (B, nbk, Hkv, D), both contiguous; `row_block0`: the global index of row block 0 (a ring rank's r * n).  Every byte of `out`
    (a torch.bool / uint8 (B, Hq, nbq, nbk) device tensor with unit last stride; None: a new one) is written."""
    _require_cuda(qbar, kbar)
    B, nbq, Hq, D = qbar.shape
    nbk, Hkv = kbar.shape[1], kbar.shape[2]
    for t, shape in ((qbar, (B, nbq, Hq, D)), (kbar, (B, nbk, Hkv, D))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"block_select: the means must be contiguous fp32 {shape} tensors, got {tuple(t.shape)} {t.dtype}")
    if out is None:
        out = torch.empty((B, Hq, nbq, nbk), dtype=torch.bool, device=qbar.device)
    elif out.dtype not in (torch.bool, torch.uint8) or tuple(out.shape) != (B, Hq, nbq, nbk) or (nbk > 1 and out.stride(-1) != 1) \
            or out.device != qbar.device:
        raise ValueError(f"block_select: out must be a torch.bool ({B}, {Hq}, {nbq}, {nbk}) tensor with unit last stride on {qbar.device}")
    _check(_feature_entry("usp_block_select")(_ptr(qbar), _ptr(kbar), B, Hq, Hkv, D, nbq, nbk, int(row_block0), float(scale),
                                              1 if causal else 0, int(top_k), int(keep_first), int(keep_local), _ptr(out),
                                              out.stride(0), out.stride(1), out.stride(2), _stream()), "usp_block_select")
    return out


def block_select_top_p_value(top_p, keep_first=0, keep_local=1, share_group=False, causal=False):
    """The checked host values of a top-p block selection (kernels/features.py: BlockSelectTopP): (top_p, keep_first, keep_local,
    share_group).  ValueError: a top_p that is no real number in (0, 1] (a bool is none, NaN is none), a keep_first / keep_local
    that is no int or negative, a share_group that is no bool, and keep_local < 1 under `causal` (no row may be left without
    its own block).  (Pure argument check.)"""
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not (0.0 < float(top_p) <= 1.0):
        raise ValueError(f"block_select: top_p must be a real number in (0, 1], got {top_p!r}")
    for name, x in (("keep_first", keep_first), ("keep_local", keep_local)):
        if isinstance(x, bool) or not isinstance(x, int):
            raise ValueError(f"block_select: {name} must be an int, got {x!r}")
        if x < 0:
            raise ValueError(f"block_select: {name} must be >= 0, got {x}")
    if not isinstance(share_group, bool):
        raise ValueError(f"block_select: share_group must be a bool, got {share_group!r}")
    if causal and keep_local < 1:
        raise ValueError(f"block_select: a causal selection needs keep_local >= 1 (every row keeps its own block), got {keep_local}")
    i32max = (1 << 31) - 1
    return float(top_p), min(keep_first, i32max), min(keep_local, i32max), share_group


def block_select_top_p(qbar, kbar, top_p, scale: float, causal: bool, keep_first: int = 0, keep_local: int = 1,
                       share_group: bool = False, row_block0: int = 0, out=None):
    """usp_block_select_top_p: the torch.bool mask (B, Hq, nbq, nbk) of the means qbar fp32 (B, nbq, Hq, D) and kbar fp32
    (B, nbk, Hkv, D), both contiguous, by cumulative softmax mass (include/usp_hip.h); `row_block0`: the global index of row
    block 0 (a ring rank's r * n).  Every byte of `out` (a torch.bool / uint8 (B, Hq, nbq, nbk) device tensor with unit last
    stride; None: a new one) is written."""
    _require_cuda(qbar, kbar)
    B, nbq, Hq, D = qbar.shape
    nbk, Hkv = kbar.shape[1], kbar.shape[2]
    for t, shape in ((qbar, (B, nbq, Hq, D)), (kbar, (B, nbk, Hkv, D))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"block_select_top_p: the means must be contiguous fp32 {shape} tensors, got {tuple(t.shape)} {t.dtype}")
    if out is None:
        out = torch.empty((B, Hq, nbq, nbk), dtype=torch.bool, device=qbar.device)
    elif out.dtype not in (torch.bool, torch.uint8) or tuple(out.shape) != (B, Hq, nbq, nbk) or (nbk > 1 and out.stride(-1) != 1) \
            or out.device != qbar.device:
        raise ValueError(f"block_select_top_p: out must be a torch.bool ({B}, {Hq}, {nbq}, {nbk}) tensor with unit last stride on {qbar.device}")
    _check(_feature_entry("usp_block_select_top_p")(_ptr(qbar), _ptr(kbar), B, Hq, Hkv, D, nbq, nbk, int(row_block0), float(scale),
                                                    1 if causal else 0, float(top_p), int(keep_first), int(keep_local),
                                                    1 if share_group else 0, _ptr(out), out.stride(0), out.stride(1), out.stride(2),
                                                    _stream()), "usp_block_select_top_p")
    return out


def block_attn_mass(q, k, lse, scale: float, causal: bool, diag: int = 0, out=None):
    """usp_block_attn_mass: the block-pooled attention map (include/usp_hip.h) of 16-bit q (B, Sq, Hq, D) and k (B, Sk, Hkv, D) with
    unit head-dim stride (kernels/attention.py: kernel_operand) and the fp32 lse (B, Hq, Sq) with unit last stride; under `causal`
    row i sees key j iff j <= i + diag.  `out`: an fp32 (B, Hq, nbq, nbk) device tensor with unit last stride -- a column slice
    of a larger result serves; None: a new one.  Every element of `out` is written."""
    _require_cuda(q, k, lse)
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    if k.shape[0] != B or k.shape[3] != D or k.dtype != q.dtype:
        raise ValueError(f"block_attn_mass: q {tuple(q.shape)} {q.dtype} and k {tuple(k.shape)} {k.dtype} do not belong together")
    if lse.dtype != torch.float32 or tuple(lse.shape) != (B, Hq, Sq):
        raise ValueError(f"block_attn_mass: lse must be an fp32 ({B}, {Hq}, {Sq}) tensor, got {tuple(lse.shape)} {lse.dtype}")
    nbq, nbk = (Sq + BLOCK_MASK_SIZE - 1) // BLOCK_MASK_SIZE, (Sk + BLOCK_MASK_SIZE - 1) // BLOCK_MASK_SIZE
    if out is None:
        out = torch.empty((B, Hq, nbq, nbk), dtype=torch.float32, device=q.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, Hq, nbq, nbk) or (nbk > 1 and out.stride(-1) != 1) \
            or out.device != q.device:
        raise ValueError(f"block_attn_mass: out must be an fp32 ({B}, {Hq}, {nbq}, {nbk}) tensor with unit last stride on {q.device}")
    tq, tk = _t4(q), _t4(k)
    lp, lsb, lsh = _lse3(lse)
    _check(_feature_entry("usp_block_attn_mass")(tq.ptr, tk.ptr, lp, dtype_code(q.dtype), B, Sq, Sk, Hq, Hkv, D, tq.stride_b,
                                                 tq.stride_s, tq.stride_h, tk.stride_b, tk.stride_s, tk.stride_h, lsb, lsh,
                                                 float(scale), 1 if causal else 0, int(diag), _ptr(out), out.stride(0),
                                                 out.stride(1), out.stride(2), _stream()), "usp_block_attn_mass")
    return out


def _feature_entries():
    """export -> (feature bit, the option as the "does not serve" message names it, argtypes) of the entry points that load()
    does not insist on."""
    i32, i64, u64, f32, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p
    fwd, bwd = ctypes.POINTER(UspFwdArgs), ctypes.POINTER(UspBwdArgs)
    return {"usp_flash_fwd_alibi": (USP_ATTN_ALIBI, "alibi_slopes (USP_ATTN_ALIBI)", [fwd, vp, i64, vp]),
            "usp_flash_bwd_alibi": (USP_ATTN_ALIBI, "alibi_slopes (USP_ATTN_ALIBI)", [bwd, vp, i64, vp]),
            "usp_flash_fwd_dropout": (USP_ATTN_DROPOUT, "dropout_p (USP_ATTN_DROPOUT)", [fwd, f32, u64, i32, i32, i32, vp]),
            "usp_flash_bwd_dropout": (USP_ATTN_DROPOUT, "dropout_p (USP_ATTN_DROPOUT)", [bwd, f32, u64, i32, i32, i32, vp]),
            "usp_flash_fwd_sink": (USP_ATTN_SINK, "sinks (USP_ATTN_SINK)", [fwd, vp, vp]),
            "usp_sink_bwd": (USP_ATTN_SINK, "sinks (USP_ATTN_SINK)", [i32, i32, i32, vp, vp, i64, i64, vp, i64, i64, vp, i32, vp]),
            "usp_flash_fwd_doc": (USP_ATTN_DOC, "cu_doclens (USP_ATTN_DOC)", [fwd, vp, i64, vp]),
            "usp_flash_bwd_doc": (USP_ATTN_DOC, "cu_doclens (USP_ATTN_DOC)", [bwd, vp, i64, vp, i64, vp]),
            "usp_flash_fwd_span": (USP_ATTN_SPAN, "bidirectional (USP_ATTN_SPAN)", [fwd, vp, i64, vp, i64, vp]),
            "usp_flash_bwd_span": (USP_ATTN_SPAN, "bidirectional (USP_ATTN_SPAN)", [bwd, vp, i64, vp, i64, vp, i64, vp, i64, vp]),
            "usp_block_list_bytes": (USP_ATTN_BLOCK_MASK, "block_mask (USP_ATTN_BLOCK_MASK)", [i32, i32, i32, i32]),
            "usp_block_lists_build": (USP_ATTN_BLOCK_MASK, "block_mask (USP_ATTN_BLOCK_MASK)",
                                      [vp, i64, i64, i64, i32, i32, i32, i32, i32, vp, vp]),
            "usp_flash_fwd_bsp": (USP_ATTN_BLOCK_MASK, "block_mask (USP_ATTN_BLOCK_MASK)", [fwd, vp, i64, i64, i64, vp, vp]),
            "usp_flash_bwd_bsp": (USP_ATTN_BLOCK_MASK, "block_mask (USP_ATTN_BLOCK_MASK)", [bwd, vp, i64, i64, i64, vp, vp]),
            "usp_flash_fwd_maxlogit": (USP_ATTN_MAX_LOGIT, "return_max_logits (USP_ATTN_MAX_LOGIT)", [fwd, vp, i64, i64, vp]),
            "usp_row_max_reduce": (USP_ATTN_MAX_LOGIT, "return_max_logits (USP_ATTN_MAX_LOGIT)", [i32, i32, i32, vp, i64, i64, vp, i32, vp]),
            "usp_block_means": (USP_ATTN_BLOCK_SELECT, "block_select (USP_ATTN_BLOCK_SELECT)", [vp, i32, i32, i32, i32, i32, i64, i64, i64, vp, vp]),
            "usp_block_select": (USP_ATTN_BLOCK_SELECT, "block_select (USP_ATTN_BLOCK_SELECT)",
                                 [vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, i32, i32, i32, i32, vp, i64, i64, i64, vp]),
            "usp_block_select_top_p": (USP_ATTN_BLOCK_SELECT_TOP_P, "block_select=BlockSelectTopP (USP_ATTN_BLOCK_SELECT_TOP_P)",
                                       [vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, i32, f32, i32, i32, i32, vp, i64, i64, i64, vp]),
            "usp_block_attn_mass": (USP_ATTN_BLOCK_MASS, "return_block_mass (USP_ATTN_BLOCK_MASS)",
                                    [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i64, i64, i64, i64, i64, i64, i64, i64, f32,
                                     i32, i32, vp, i64, i64, i64, vp])}


_FEATURE_ENTRIES = _feature_entries()


def _feature_entry(name: str):
    """The entry point `name` of _FEATURE_ENTRIES, prototyped on first use; a library without the feature bit (built before
    the entry points: it loads, they are not insisted on) is refused."""
    bit, option, argtypes = _FEATURE_ENTRIES[name]
    L = load()
    if not (hasattr(L, "usp_attn_features") and L.usp_attn_features() & bit and hasattr(L, name)):
        raise NotImplementedError(f"{_LIB_PATH} does not serve {option}: rebuild it")
    fn = getattr(L, name)
    if fn.argtypes is None:
        fn.argtypes = argtypes
        fn.restype = ctypes.c_int64 if name == "usp_block_list_bytes" else ctypes.c_int
    return fn


_alibi_entry = _dropout_entry = _sink_entry = _doc_entry = _span_entry = _bsp_entry = _maxl_entry = _select_entry = _select_top_p_entry = _mass_entry = _feature_entry      # (the names the per-feature tests call it by)


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _set_shift(a, shift: Optional[int]):
    """Set USP_ATTN_SHIFT + the field on an argument block (None = off); a library that does not report the bit would
    ignore it silently and compute another mask, so it is refused here."""
    if shift is None:
        return
    L = load()
    if not (hasattr(L, "usp_attn_features") and L.usp_attn_features() & USP_ATTN_SHIFT):
        raise RuntimeError(f"{_LIB_PATH} does not serve a mask shift (USP_ATTN_SHIFT): rebuild it")
    a.flags |= USP_ATTN_SHIFT
    a.mask_shift = int(shift)


def _shift(shift) -> Optional[int]:
    """`shift` argument -> int, or None when it is off.  (0 is a valid shift and sets the bit: the call decodes like an
    unshifted one.)"""
    if shift is None:
        return None
    s = int(shift)
    if abs(s) >= 1 << 30:
        raise ValueError(f"shift must lie inside (-2^30, 2^30), got {shift!r}")
    return s


def _flash_call(which: str, a, al, dr, sk, dc, sp=None, mx=None):
    """Issues the flash launch `which` ("fwd" | "bwd") of the filled argument block `a` with the decoded extras (alibi_value,
    dropout_args, sinks_value, doc_value, span_value; None = off): through the entry point of the one that is on -- two of them
    are refused (kernels/features.py) -- or the plain one.  `mx`: the forward's buffer of row maxima (row_max_value), which goes
    with none of the others."""
    if mx is not None:
        _maxl_alone(alibi=al, dropout=dr, sinks=sk, doc=dc, span=sp)
        name = "usp_flash_fwd_maxlogit"
        _check(_feature_entry(name)(ctypes.byref(a), *mx, _stream()), name)
        return
    if sp is not None:
        from .kernels.features import Features
        from .kernels.features import SPAN_ON
        Features(alibi=al, dropout=dr, sinks=sk, doc=SPAN_ON).check()
        if dc is not None:
            raise ValueError("a launch takes doc= or span=, not both: the span arrays hold the document bound")
        (rl, rl_sb), (rh, rh_sb), (kl, kl_sb), (kh, kh_sb) = sp
        name = f"usp_flash_{which}_span"             # (the forward reads the row arrays alone)
        extra = (_ptr(rl), rl_sb, _ptr(rh), rh_sb) + (() if which == "fwd" else (_ptr(kl), kl_sb, _ptr(kh), kh_sb))
        _check(_feature_entry(name)(ctypes.byref(a), *extra, _stream()), name)
        return
    if al is None and dr is None and sk is None and dc is None:
        name, extra = "usp_flash_" + which, ()
        fn = getattr(load(), name)
    else:
        from .kernels.features import Features
        Features(alibi=al, dropout=dr, sinks=sk, doc=dc).check()
        if dc is not None:
            (rl, rl_sb), (kh, kh_sb) = dc
            name = f"usp_flash_{which}_doc"          # (the forward reads row_lo alone)
            extra = (_ptr(rl), rl_sb) if which == "fwd" else (_ptr(rl), rl_sb, _ptr(kh), kh_sb)
        elif sk is not None:
            name, extra = "usp_flash_fwd_sink", (_ptr(sk),)
        elif dr is not None:
            name, extra = f"usp_flash_{which}_dropout", dr
        else:
            name, extra = f"usp_flash_{which}_alibi", (_ptr(al[0]), al[1])
        fn = _feature_entry(name)
    _check(fn(ctypes.byref(a), *extra, _stream()), name)


def _fwd_args(q, k, v, softmax_scale, causal, lse, out, acc, merge_in, final_begin, final_end, interleave, n, window=None,
              family_flag=0, softcap=None, shift=None):
    """The filled usp_fwd_args block of a dense launch.  Everything but the seven pointers is a function of
    (dtype, shapes, strides, flags), and a training loop issues the same few launches over and over: the block is
    cached per thread under that signature and only the pointers are patched (filling 27 ctypes fields and five
    usp_tensor structs costs ~35 us of host time per launch, tools/host_step_cpu.py; a hit costs ~8)."""
    key = (q.dtype, q.shape, q.stride(), k.shape, k.stride(), v.stride(), lse.stride(), _strides(out), _strides(acc),
           softmax_scale, causal, merge_in, final_begin, final_end, interleave, n, window, family_flag, softcap, shift)
    cache = _TLS.__dict__.setdefault("fwd", {})
    a = cache.get(key)
    if a is None:
        B, Sq, Hq, D = q.shape
        a = UspFwdArgs()
        a.dtype = dtype_code(q.dtype)
        a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D = B, Sq, k.shape[1], Hq, k.shape[2], D
        a.causal = 1 if causal else 0
        a.softmax_scale = float(softmax_scale)
        a.q, a.k, a.v, a.out, a.acc = _t4(q), _t4(k), _t4(v), _t4(out), _t4(acc)
        a.lse, a.lse_stride_b, a.lse_stride_h = _lse3(lse)
        a.merge_in = 1 if merge_in else 0
        a.final_begin = final_begin
        a.final_end = Sq if final_end is None else final_end
        a.flags = (USP_LAUNCH_INTERLEAVE if interleave else 0) | family_flag
        if window is not None:
            a.flags |= USP_ATTN_WINDOW
            a.window_left, a.window_right = window
        _set_softcap(a, softcap)
        _set_shift(a, shift)
        a.k_splits = n if n > 1 else 0
        if len(cache) >= _ARGS_CACHE_MAX:
            cache.clear()
        cache[key] = a
        return a
    a.q.ptr, a.k.ptr, a.v.ptr, a.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), lse.data_ptr()
    a.out.ptr = None if out is None else out.data_ptr()
    a.acc.ptr = None if acc is None else acc.data_ptr()
    return a


def flash_fwd(q, k, v, softmax_scale: float, causal: bool, lse, out=None, acc=None,
              merge_in: bool = False, final_begin: int = 0, final_end: Optional[int] = None,
              interleave: bool = False, k_splits: Optional[int] = None, window=None, family=None, softcap=None, shift=None,
              alibi=None, dropout=None, sinks=None, doc=None, span=None, bsp=None, bsp_lists=None, row_max=None):
    """usp_flash_fwd (include/usp_hip.h).  q (B,Sq,Hq,D); k,v (B,Sk,Hkv,D); lse (B,Hq,Sq) fp32;
    out 16-bit / acc fp32 (B,Sq,Hq,D).  All may be strided views (unit dim stride).  `k_splits`: cut the keys of
    every query tile into that many work items (None: fwd_k_splits decides; 0 / 1: off).  `window` = flash-attn's
    window_size (left, right), None / (-1, -1) = none.  `family`: "row64" | "wave32" pins the kernel family of this call
    (ABI v6; None: set_kernel_family's default, normally "auto"); both families serve a K split.  `softcap`: flash-attn's
    logit soft-capping, None / 0 = off (softcap_value; the 64-row family declines it: family="row64" then fails).
    `shift` (None | int, USP_ATTN_SHIFT): moves the diagonal of the causal and window bounds, row i sees key j iff
    i + (Sk - Sq + shift) - left <= j <= i + (Sk - Sq + shift) + right -- the mask of one block of a ring (ring/window_blocks.py).
    A shifted launch gets no automatic K split (fwd_k_splits sizes cuts for a causal triangle).
    `alibi`: flash-attn's alibi_slopes, fp32 (Hq,) or (B, Hq) on q's device (alibi_value), None = off: the score of (row i,
    key j) gets -slope * |i + (Sk - Sq + shift) - j| before the mask (usp_flash_fwd_alibi; not with softcap or family="row64").
    `dropout`: (p, seed, row0, key0, head0) (dropout_args), None = off: the probabilities are dropped by the position-keyed
    mask of include/usp_hip.h and the kept ones rescaled (usp_flash_fwd_dropout; not with softcap, alibi or family="row64").
    `sinks`: one learned logit per query head (sinks_value), None = off: it joins every row's softmax denominator and carries no
    value; `lse` includes it (usp_flash_fwd_sink; a launch without merge_in only; not with softcap, alibi, dropout or
    family="row64").
    `doc`: (row_lo, key_hi) int32 device arrays (doc_value), None = off: row i sees key j only if j >= row_lo[i], the document
    mask of one launch (usp_flash_fwd_doc; served uncut; not with window, softcap, shift, alibi, dropout, sinks or family="row64").
    `span`: (row_lo, row_hi, key_lo, key_hi) int32 device arrays (span_value), None = off: row i sees key j only if
    row_lo[i] <= j < row_hi[i], the mask of one launch under bidirectional spans with the diagonal folded into row_hi
    (usp_flash_fwd_span; causal=False only; served uncut; not with doc or anything doc refuses).
    `bsp`: a torch.bool block mask (block_mask_value) of this launch's BLOCK_MASK_SIZE-square blocks, None = off: row i sees key j
    only if bsp[b, h, i // 128, j // 128] (usp_flash_fwd_bsp; Sq == Sk; served uncut; not with any other option above but causal).  `bsp_lists`: the scratch of its lists
    (block_list_bytes, block_list_layout; None: allocated here).
    `row_max`: an fp32 (B, Hq, Sq) device tensor with unit seq stride (row_max_value), None = off: receives the largest visible
    softmax_scale * q.k of every row, -inf where a row sees nothing; with merge_in the maximum with the value there
    (usp_flash_fwd_maxlogit; served uncut, k_splits ignored; goes with window and shift alone; not with family="row64")."""
    _require_cuda(q, k, v, lse, out, acc, row_max)
    B, Sq, Hq, D = q.shape
    mx = row_max_value(row_max, B, Hq, Sq, q.device)
    bm = block_mask_value(bsp, B, Hq, Sq, q.device)
    if mx is not None:
        _maxl_alone(softcap=softcap_value(softcap), bsp=bm)
    if bm is not None:
        _bsp_alone(window=_window(window), softcap=softcap_value(softcap), shift=_shift(shift), alibi=alibi, dropout=dropout_args(dropout),
                   sinks=sinks, doc=doc_value(doc, B, Sq, k.shape[1], q.device), span=span_value(span, B, Sq, k.shape[1], q.device))
        a = _fwd_args(q, k, v, softmax_scale, bool(causal), lse, out, acc, bool(merge_in), final_begin, final_end,
                      bool(interleave), 0, None, _family_flag(family), None, None)
        _bsp_call("fwd", a, bm, bsp_lists)
        return
    cap = softcap_value(softcap)
    ff = _family_flag(family)
    win, sh = _window(window), _shift(shift)
    dc = doc_value(doc, B, Sq, k.shape[1], q.device)     # None: off -- (None, None) included, which is the call without the keyword
    sp = span_value(span, B, Sq, k.shape[1], q.device)   # None: off, likewise
    if k_splits is None:
        n = 0 if (sh is not None or dc is not None or sp is not None or mx is not None) else fwd_k_splits(B, Sq, Hq, causal)   # (a document or max-logit launch is served uncut)
    else:
        n = int(k_splits)
    a = _fwd_args(q, k, v, softmax_scale, bool(causal), lse, out, acc, bool(merge_in), final_begin, final_end,
                  bool(interleave), n, win, ff, cap, sh)
    L = load()
    if n > 1:
        # scratch for the partial results: one buffer per (device, stream), grown on demand; launches on one stream
        # are ordered, so the buffer is free again when the next launch on that stream starts
        need = L.usp_flash_fwd_workspace_bytes(ctypes.byref(a), n)
        key = (q.device.index, torch.cuda.current_stream().cuda_stream)
        ws = _FWD_WS.get(key)
        if ws is None or ws.numel() < need:
            ws = _FWD_WS[key] = torch.empty(need, dtype=torch.uint8, device=q.device)
        a.workspace = ws.data_ptr()
    al = alibi_value(alibi, B, Hq, q.device)
    dr = dropout_args(dropout)
    sk = sinks_value(sinks, Hq, q.device, q.dtype)
    _flash_call("fwd", a, al, dr, sk, dc, sp, mx)


def _maxl_alone(**others):
    """A max-logit launch takes no other option but a window and a shift: the entry point has no second extra."""
    for name, value in others.items():
        if value is not None:
            raise NotImplementedError(f"row_max together with {name} is not supported by the HIP attention kernels")


def row_max_value(row_max, B: int, Hq: int, Sq: int, device):
    """A `row_max` argument -> (pointer, batch stride, head stride) as usp_flash_fwd_maxlogit / usp_row_max_reduce take it, or None
    when it is off."""
    if row_max is None:
        return None
    if not isinstance(row_max, torch.Tensor) or row_max.dtype != torch.float32:
        raise ValueError("row_max must be a float32 torch.Tensor")
    if tuple(row_max.shape) != (B, Hq, Sq):
        raise ValueError(f"row_max must have shape ({B}, {Hq}, {Sq}): one value per (batch, query head, row), got {tuple(row_max.shape)}")
    if row_max.device != torch.device(device):
        raise ValueError(f"row_max is on {row_max.device}, the operands on {device}")
    return _lse3(row_max)


def row_max_reduce(row_max, out=None, accum: bool = False):
    """usp_row_max_reduce: out[h] = max_{b,i} row_max[b,h,i] (with `accum`: and of out[h]) of an fp32 (B,H,S) tensor with unit seq
    stride.  `out`: an fp32 contiguous (H,) buffer (None: a new one).  Returns it.  Exact, deterministic, no host read."""
    _require_cuda(row_max, out)
    B, H, S = row_max.shape
    mx = row_max_value(row_max, B, H, S, row_max.device)
    if out is None:
        if accum:
            raise ValueError("row_max_reduce: accum needs the buffer to take the maximum with")
        out = torch.empty(H, dtype=torch.float32, device=row_max.device)
    if out.dtype != torch.float32 or tuple(out.shape) != (H,) or not out.is_contiguous():
        raise ValueError("row_max_reduce: out must be a contiguous float32 (H,) tensor")
    _check(_feature_entry("usp_row_max_reduce")(B, S, H, *mx, _ptr(out), 1 if accum else 0, _stream()), "usp_row_max_reduce")
    return out


def _bsp_alone(**others):
    """A block-sparse launch takes no other option: the entry point has no second extra and declines the flag bits."""
    for name, value in others.items():
        if value is not None:
            raise NotImplementedError(f"bsp together with {name} is not supported by the HIP attention kernels")


def _t3(t: Optional[torch.Tensor]) -> UspTensor:
    """(T,H,D) token tensor with unit dim stride -> usp_tensor (batch stride unused)."""
    if t is None:
        return UspTensor(None, 0, 0, 0)
    assert t.dim() == 3, t.shape
    if t.stride(2) != 1:
        raise ValueError("last (head_dim) stride must be 1")
    return UspTensor(t.data_ptr(), 0, t.stride(0), t.stride(1))


def _lse2(t: torch.Tensor):
    """(H,T) fp32 with unit token stride -> (ptr, 0, stride_h)."""
    assert t.dim() == 2 and t.dtype == torch.float32
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError("lse/delta must have unit stride along the tokens")
    return ctypes.c_void_p(t.data_ptr()), 0, t.stride(0)


def _seq(t: torch.Tensor, n: int) -> ctypes.c_void_p:
    """(n,2) int32 device tensor of (first_row, rows) pairs."""
    if t.dtype != torch.int32 or tuple(t.shape) != (n, 2) or not t.is_contiguous():
        raise ValueError("sequence table must be a contiguous (num_seq, 2) int32 tensor")
    _require_cuda(t)
    return ctypes.c_void_p(t.data_ptr())


_SCHED = {}


def sched_block(device) -> torch.Tensor:
    """The 16-int32 control block of the packed kernels' dynamic item queue (include/usp_hip.h `sched`):
    zeroed once, left zeroed by every launch, one per (device, stream) because launches on different
    streams may overlap."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    blk = _SCHED.get(key)
    if blk is None:
        blk = _SCHED[key] = torch.zeros(16, dtype=torch.int32, device=device)
    return blk


def flash_fwd_packed(q, k, v, seq_q, seq_k, max_q: int, max_k: int, softmax_scale: float,
                     causal: bool, lse, out=None, acc=None, merge_in: bool = False,
                     final_begin: int = 0, final_end: int = 2, interleave: bool = False, softcap=None, sched: bool = True):
    """usp_flash_fwd in packed variable-length mode.  q/out/acc (T,Hq,D), k/v (T',Hkv,D), lse (Hq,T)
    fp32; seq_q/seq_k (num_seq,2) int32 device tables of (first_row, rows); final_begin/final_end
    count half sequences (0,1,2); `softcap` as flash_fwd.  `sched=False` passes no control block: the workgroups walk their
    static item lists instead of the dynamic queue (include/usp_hip.h `sched`; tests and A/B runs)."""
    _require_cuda(q, k, v, lse, out, acc)
    cap = softcap_value(softcap)
    n = seq_q.shape[0]
    a = UspFwdArgs()
    a.dtype = dtype_code(q.dtype)
    a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D = n, int(max_q), int(max_k), q.shape[1], k.shape[1], q.shape[2]
    a.causal = 1 if causal else 0
    a.softmax_scale = float(softmax_scale)
    a.q, a.k, a.v, a.out, a.acc = _t3(q), _t3(k), _t3(v), _t3(out), _t3(acc)
    a.lse, a.lse_stride_b, a.lse_stride_h = _lse2(lse)
    a.merge_in = 1 if merge_in else 0
    a.final_begin, a.final_end = int(final_begin), int(final_end)
    a.seq_q, a.seq_k = _seq(seq_q, n), _seq(seq_k, n)
    a.sched = sched_block(q.device).data_ptr() if sched else None
    a.flags = USP_LAUNCH_INTERLEAVE if interleave else 0
    _set_softcap(a, cap)
    _check(load().usp_flash_fwd(ctypes.byref(a), _stream()), "usp_flash_fwd")


def flash_bwd_packed(dout, q, k, v, lse, delta, seq_q, seq_k, max_q: int, max_k: int, dq, dk, dv,
                     softmax_scale: float, causal: bool, accum_dq=False, accum_dk=False,
                     accum_dv=False, dq16=None, dk16=None, dv16=None, interleave: bool = False, softcap=None,
                     sched: bool = True):
    """usp_flash_bwd in packed variable-length mode (layouts as flash_fwd_packed; lse/delta (Hq,T); `softcap` and `sched`
    as flash_fwd_packed)."""
    _require_cuda(dout, q, k, v, lse, delta, dq, dk, dv, dq16, dk16, dv16)
    cap = softcap_value(softcap)
    n = seq_q.shape[0]
    a = UspBwdArgs()
    a.dtype = dtype_code(q.dtype)
    a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D = n, int(max_q), int(max_k), q.shape[1], k.shape[1], q.shape[2]
    a.causal = 1 if causal else 0
    a.softmax_scale = float(softmax_scale)
    a.dout, a.q, a.k, a.v = _t3(dout), _t3(q), _t3(k), _t3(v)
    a.lse, a.lse_stride_b, a.lse_stride_h = _lse2(lse)
    a.delta, a.delta_stride_b, a.delta_stride_h = _lse2(delta)
    for t in (dq, dk, dv):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("dq/dk/dv buffers of usp_flash_bwd are fp32")
    a.dq, a.dk, a.dv = _t3(dq), _t3(dk), _t3(dv)
    a.dq16, a.dk16, a.dv16 = _t3(dq16), _t3(dk16), _t3(dv16)
    a.accum_dq, a.accum_dk, a.accum_dv = int(bool(accum_dq)), int(bool(accum_dk)), int(bool(accum_dv))
    a.seq_q, a.seq_k = _seq(seq_q, n), _seq(seq_k, n)
    a.sched = sched_block(q.device).data_ptr() if sched else None
    a.flags = USP_LAUNCH_INTERLEAVE if interleave else 0
    _set_softcap(a, cap)
    a.total_k = k.shape[0]
    L = load()
    need = L.usp_flash_bwd_workspace_bytes(ctypes.byref(a))
    ws = None
    if need > 0:
        ws = torch.empty(need, dtype=torch.uint8, device=q.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
    _check(L.usp_flash_bwd(ctypes.byref(a), _stream()), "usp_flash_bwd")


def bwd_delta(dout, out, delta):
    _require_cuda(dout, out, delta)
    B, S, H, D = dout.shape
    td, to = _t4(dout), _t4(out)
    p, sb, sh = _lse3(delta)
    _check(load().usp_bwd_delta(dtype_code(dout.dtype), B, S, H, D, ctypes.byref(td),
                                ctypes.byref(to), p, sb, sh, _stream()), "usp_bwd_delta")


def sink_grad(sinks, lse, delta, out=None, accum: bool = False):
    """usp_sink_bwd: out[h] (+)= -sum_{b,i} exp(sinks[h] - lse[b,h,i]) * delta[b,h,i], the gradient of the sink logits from the
    sink-including `lse` and the backward's `delta` (both (B,H,S) fp32, unit seq stride).  `out`: an fp32 contiguous (H,) buffer
    (None: a new one), added to with `accum`.  Returns it.  fp32, deterministic."""
    _require_cuda(sinks, lse, delta, out)
    B, H, S = lse.shape
    assert delta.shape == lse.shape, (delta.shape, lse.shape)
    sk = sinks_value(sinks, H, lse.device)
    if out is None:
        if accum:
            raise ValueError("sink_grad: accum needs the buffer to add to")
        out = torch.empty(H, dtype=torch.float32, device=lse.device)
    if out.dtype != torch.float32 or tuple(out.shape) != (H,) or not out.is_contiguous():
        raise ValueError("sink_grad: out must be a contiguous float32 (H,) tensor")
    pl, lsb, lsh = _lse3(lse)
    pd, dsb, dsh = _lse3(delta)
    _check(_feature_entry("usp_sink_bwd")(B, S, H, ctypes.c_void_p(sk.data_ptr()), pl, lsb, lsh, pd, dsb, dsh,
                                       ctypes.c_void_p(out.data_ptr()), 1 if accum else 0, _stream()), "usp_sink_bwd")
    return out


def flash_bwd(dout, q, k, v, lse, delta, dq, dk, dv, softmax_scale: float, causal: bool,
              accum_dq=False, accum_dk=False, accum_dv=False, dq16=None, dk16=None, dv16=None,
              interleave: bool = False, splits=None, window=None, family=None, only=None, dkdv_heads: int = 0,
              softcap=None, shift=None, alibi=None, dropout=None, doc=None, span=None, bsp=None, bsp_lists=None, dkdv_keys: int = 0):
    """usp_flash_bwd.  dq/dk/dv are fp32 (B,S,H,D) views, written or accumulated; a 16-bit
    dq16/dk16/dv16 receives the FINAL rounded result instead (the fp32 tensor may then be None
    unless it is accumulated from).  `splits` = (dq_splits, dkdv_splits), None: bwd_splits decides.  `window` =
    flash-attn's window_size (left, right), None / (-1, -1) = none.  `family`: as flash_fwd.  `only`: "dkdv" | "dq" issues
    just that launch of the two (ABI v6: USP_BWD_SKIP_DQ / USP_BWD_SKIP_DKDV).  `dkdv_heads` (ABI v7): query heads of a KV
    group one dK/dV work item streams (a divisor of Hq / Hkv; 0 = the library decides).  `softcap`, `shift`: as flash_fwd (a
    shifted launch gets no automatic cuts: bwd_splits sizes them for a causal triangle).  `alibi`: as flash_fwd
    (usp_flash_bwd_alibi).  `dropout`: as flash_fwd (usp_flash_bwd_dropout): the same tuple regenerates the forward's mask;
    `delta` is that of the dropped `out`.  `dkdv_keys`: 128 | 256 pins the item width of the 64-row dK/dV kernel (USP_DKDV_KEYS128 /
    USP_DKDV_KEYS256; 0: the library picks; last_dkdv_item_keys() tells which ran).  `doc`: as flash_fwd (usp_flash_bwd_doc): the dQ launch reads row_lo, the dK/dV launch
    key_hi; with `only` the other one may be None.  `span`: as flash_fwd (usp_flash_bwd_span): the dQ launch reads (row_lo,
    row_hi), the dK/dV launch (key_lo, key_hi); with `only` the other pair may be None.  `bsp`: as flash_fwd (usp_flash_bwd_bsp)."""
    _require_cuda(dout, q, k, v, lse, delta, dq, dk, dv, dq16, dk16, dv16)
    cap = softcap_value(softcap)
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    a = UspBwdArgs()
    a.dtype = dtype_code(q.dtype)
    a.B, a.Sq, a.Sk, a.Hq, a.Hkv, a.D = B, Sq, Sk, Hq, Hkv, D
    a.causal = 1 if causal else 0
    a.softmax_scale = float(softmax_scale)
    a.dout, a.q, a.k, a.v = _t4(dout), _t4(q), _t4(k), _t4(v)
    a.lse, a.lse_stride_b, a.lse_stride_h = _lse3(lse)
    a.delta, a.delta_stride_b, a.delta_stride_h = _lse3(delta)
    for t in (dq, dk, dv):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("dq/dk/dv buffers of usp_flash_bwd are fp32")
    a.dq, a.dk, a.dv = _t4(dq), _t4(dk), _t4(dv)
    a.dq16, a.dk16, a.dv16 = _t4(dq16), _t4(dk16), _t4(dv16)
    a.accum_dq, a.accum_dk, a.accum_dv = int(bool(accum_dq)), int(bool(accum_dk)), int(bool(accum_dv))
    ff = _family_flag(family)
    a.flags = (USP_LAUNCH_INTERLEAVE if interleave else 0) | ff | {None: 0, "dkdv": USP_BWD_SKIP_DQ, "dq": USP_BWD_SKIP_DKDV}[only]
    if dkdv_keys not in _DKDV_KEYS_FLAG:
        raise ValueError(f"dkdv_keys must be 0, 128 or 256, got {dkdv_keys!r}")
    a.flags |= _DKDV_KEYS_FLAG[dkdv_keys]
    sh = _shift(shift)
    dc = doc_value(doc, B, Sq, Sk, q.device)             # None: off -- (None, None) included
    sp = span_value(span, B, Sq, Sk, q.device)
    bm = block_mask_value(bsp, B, Hq, Sq, q.device)
    if bm is not None:
        _bsp_alone(window=_window(window), softcap=cap, shift=sh, alibi=alibi, dropout=dropout_args(dropout), doc=dc, span=sp)
    if splits is None:
        a.dq_splits, a.dkdv_splits = (0, 0) if (sh is not None or dc is not None or sp is not None or bm is not None) else bwd_splits(B, Sq, Sk, Hq, bool(causal))
    else:
        a.dq_splits, a.dkdv_splits = splits
    a.dkdv_heads = int(dkdv_heads)
    win = _window(window)
    if win is not None:
        a.flags |= USP_ATTN_WINDOW
        a.window_left, a.window_right = win
    _set_softcap(a, cap)
    _set_shift(a, sh)
    L = load()
    need = L.usp_flash_bwd_workspace_bytes(ctypes.byref(a))     # GQA head split and / or cuts of few-item launches
    ws = None
    if need > 0:
        ws = torch.empty(need, dtype=torch.uint8, device=q.device)   # caching allocator; stream-ordered
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
    if bm is not None:
        _bsp_call("bwd", a, bm, bsp_lists)
        return
    al = alibi_value(alibi, B, Hq, q.device)
    dr = dropout_args(dropout)
    _flash_call("bwd", a, al, dr, None, dc, sp)


def lse_merge(acc, lse, blk_out, blk_lse, first: bool):
    _require_cuda(acc, lse, blk_out, blk_lse)
    B, S, H, D = acc.shape
    ta, tb = _t4(acc), _t4(blk_out)
    p, sb, sh = _lse3(lse)
    p2, sb2, sh2 = _lse3(blk_lse)
    _check(load().usp_lse_merge(dtype_code(blk_out.dtype), B, S, H, D, ctypes.byref(ta), p, sb, sh,
                                ctypes.byref(tb), p2, sb2, sh2, 1 if first else 0, _stream()),
           "usp_lse_merge")


def copy_rows(dst, src, row_bytes, sizes, dst_strides, src_strides):
    """usp_copy_rows: strides in BYTES, 4 outer dims."""
    _require_cuda(dst, src)
    n = list(sizes) + [1] * (4 - len(sizes))
    ds = list(dst_strides) + [0] * (4 - len(dst_strides))
    ss = list(src_strides) + [0] * (4 - len(src_strides))
    _check(load().usp_copy_rows(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()),
                                row_bytes, *n, *ds, *ss, _stream()), "usp_copy_rows")


def sum_rows(dst, src, row_bytes, r, term_stride, sizes, dst_strides, src_strides):
    """usp_sum_rows: dst rows = round(sum of r source rows `term_stride` bytes apart), fp32 in ascending term order.
    Strides in BYTES, up to 3 outer dims; dst and src of one 16-bit dtype."""
    _require_cuda(dst, src)
    if dst.dtype != src.dtype:
        raise TypeError(f"usp_sum_rows: dst {dst.dtype} and src {src.dtype} differ")
    if len(sizes) > 3 or len(dst_strides) != len(sizes) or len(src_strides) != len(sizes):
        raise ValueError(f"usp_sum_rows takes up to 3 outer dims with one stride each: {sizes} {dst_strides} {src_strides}")
    n = list(sizes) + [1] * (3 - len(sizes))
    ds = list(dst_strides) + [0] * (3 - len(dst_strides))
    ss = list(src_strides) + [0] * (3 - len(src_strides))
    _check(load().usp_sum_rows(dtype_code(dst.dtype), ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()),
                               int(row_bytes), int(r), int(term_stride), *n, *ds, *ss, _stream()), "usp_sum_rows")


def _rows2d(t: torch.Tensor):
    """View a tensor as `rows` rows of `n` contiguous elements with one row stride."""
    if t.is_contiguous():
        return 1, t.numel(), t.numel()
    if t.dim() == 4 and t[0].is_contiguous():          # (B, ...) slices of a bigger batch stride
        return t.shape[0], t[0].numel(), t.stride(0)
    raise ValueError("expected a contiguous tensor or a batch of contiguous slices")


def cast_from_f32(dst16, src32):
    _require_cuda(dst16, src32)
    r1, n1, s1 = _rows2d(dst16)
    r2, n2, s2 = _rows2d(src32)
    if (r1, n1) != (r2, n2):
        r1, n1, s1, s2 = dst16.shape[0], dst16[0].numel(), dst16.stride(0), src32.stride(0)
        assert dst16[0].is_contiguous() and src32[0].is_contiguous()
    _check(load().usp_cast_from_f32(dtype_code(dst16.dtype), ctypes.c_void_p(dst16.data_ptr()), s1,
                                    ctypes.c_void_p(src32.data_ptr()), s2, r1, n1, _stream()),
           "usp_cast_from_f32")


def add_f32(dst, a, b):
    """dst = a + b (fp32), tensors contiguous or batches of contiguous slices of equal shape."""
    _require_cuda(dst, a, b)
    assert dst.shape == a.shape == b.shape
    if dst.is_contiguous() and a.is_contiguous() and b.is_contiguous():
        rows, n, sd, sa, sb_ = 1, dst.numel(), dst.numel(), a.numel(), b.numel()
    else:
        assert dst[0].is_contiguous() and a[0].is_contiguous() and b[0].is_contiguous()
        rows, n = dst.shape[0], dst[0].numel()
        sd, sa, sb_ = dst.stride(0), a.stride(0), b.stride(0)
    _check(load().usp_add_f32(ctypes.c_void_p(dst.data_ptr()), sd, ctypes.c_void_p(a.data_ptr()), sa,
                              ctypes.c_void_p(b.data_ptr()), sb_, rows, n, _stream()), "usp_add_f32")


def mfma_probe(operands: torch.Tensor, iters: int, waves_per_simd: int = 1, clocks: Optional[torch.Tensor] = None):
    """usp_mfma_probe: one launch of the MFMA-only loop on `operands` (a bf16 device tensor of >= 32768 elements).
    Returns the FLOPs of the launch; `clocks`: optional int64[2] device tensor (shader-clock and 100 MHz ticks)."""
    _require_cuda(operands, clocks)
    assert operands.dtype == torch.bfloat16 and operands.is_contiguous() and operands.numel() >= 32768
    key = ("probe_sink", operands.device.index)
    sink = _SCHED.get(key)
    if sink is None:
        sink = _SCHED[key] = torch.zeros(512, dtype=torch.float32, device=operands.device)
    _check(load().usp_mfma_probe(ctypes.c_void_p(operands.data_ptr()), operands.numel() * 2, int(iters), int(waves_per_simd),
                                 ctypes.c_void_p(sink.data_ptr()), ctypes.c_void_p(clocks.data_ptr() if clocks is not None else None),
                                 _stream()), "usp_mfma_probe")
    cus = torch.cuda.get_device_properties(operands.device).multi_processor_count
    return cus * 4 * waves_per_simd * iters * 64 * 32768.0
