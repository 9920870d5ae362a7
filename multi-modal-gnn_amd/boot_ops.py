"""ctypes binding and typed entry points of libmmgnn_boot.so (C ABI: include/mmgnn_boot.h; csrc/boot.hip): the weighted
segment sums of the patient-cluster bootstrap, the metrics of every replicate and their summary, a library of its own
beside libmmgnn.so.  The binding is derived from the header by the same parser as _lib's (``_lib.parse_header``) and the
calls are marshalled from the prototypes as ``conformal_ops._call`` marshals them.  The library is REQUIRED: there is no
CPU or eager-PyTorch fallback behind these calls (the numpy restatement of mmgnn/bootstrap.py serves numpy inputs and
checks the kernels; it is never a silent substitute for them).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _lib, ops
from ._lib import MmgError, check

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmmgnn_boot.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mmgnn_boot.h")


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise MmgError(f"{HEADER_PATH} not found: the binding is derived from the header the library is built from "
                       f"({e})") from None


PARAMS = {}
DEFINES, STRUCTS, SIGNATURES = _lib.parse_header(_read_header(), PARAMS)
globals().update(DEFINES)
_PLANS = {sym: ops._plan(params) for sym, params in PARAMS.items()}

BOOT_SITE = DEFINES["MMG_BOOT_SITE"]
BOOT_MAX_REPLICATES = DEFINES["MMG_BOOT_MAX_REPLICATES"]
BOOT_MAX_SEG = DEFINES["MMG_BOOT_MAX_SEG"]
BOOT_CHUNK = DEFINES["MMG_BOOT_CHUNK"]                  # C: sorted pairs per chunk
BOOT_RB = DEFINES["MMG_BOOT_RB"]                        # RB: replicates per workgroup
BOOT_DROP_KINDS = DEFINES["MMG_BOOT_DROP_KINDS"]        # segment out of range, unit out of range, NaN value
BOOT_FIELDS = DEFINES["MMG_BOOT_FIELDS"]
BOOT_FIELDS_B = DEFINES["MMG_BOOT_FIELDS_B"]
BOOT_METRICS = DEFINES["MMG_BOOT_METRICS"]
BOOT_METRICS_B = DEFINES["MMG_BOOT_METRICS_B"]
BOOT_SUMMARY_FIELDS = DEFINES["MMG_BOOT_SUMMARY_FIELDS"]

_btlib = None


def load():
    """Load libmmgnn_boot.so (once), after libmmgnn.so, which it uses.  Raises MmgError loudly when it has not been
    built."""
    global _btlib
    if _btlib is not None:
        return _btlib
    _lib.load()
    if not os.path.exists(LIB_PATH):
        raise MmgError(f"{LIB_PATH} not found: the HIP library is mandatory (no CPU fallback). Build it with "
                       f"`make -C {os.path.join(_HERE, 'csrc')}` or `python -c 'import __graft_entry__ as g; g.build()'`.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)     # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _btlib = lib
    return lib


def _call(name, *args, ws=None):
    """conformal_ops._call for this library: `args` are the parameters of the prototype of `name` without stream, ws and
    ws_bytes; a torch.Tensor handed to a scalar pointer parameter is converted under the header's dtype and name, tensors
    on different devices are refused; ws: the call's uint8 workspace tensor."""
    plan, n_given = _PLANS[name]
    if len(args) != n_given:
        raise TypeError(f"{name}: takes {n_given} arguments besides ws and stream, got {len(args)}")
    out, dev, given = [], None, iter(args)
    for how in plan:
        a = (0 if how == "ws_bytes" else None) if isinstance(how, str) else next(given)
        if how is not None and isinstance(a, torch.Tensor):
            t, a = a, ops._p(a, how[1], how[0])
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise ValueError(f"{name}: {how[0]} is on {t.device}, the tensors before it on {dev}")
        out.append(a)
    for i, how in enumerate(plan):
        if how == "stream":
            out[i] = ops._stream()
        elif how == "ws" and ws is not None:
            out[i], out[i + 1] = ops._p(ws, torch.uint8, "ws"), ws.numel()
    check(getattr(load(), name)(*out), name)


def _ws(nbytes: int, device):
    return ops.workspace(max(int(nbytes), 256), device)


def n_fields(with_b: bool) -> int:
    return BOOT_FIELDS_B if with_b else BOOT_FIELDS


def n_metrics(with_b: bool) -> int:
    return BOOT_METRICS_B if with_b else BOOT_METRICS


def boot_sums(pred: torch.Tensor, target: torch.Tensor, unit: torch.Tensor, seg: torch.Tensor, n_units: int, n_seg: int,
              replicates: int, seed: int = 0, pred_b: Optional[torch.Tensor] = None, out=None):
    """The weighted segment sums of every replicate (mmg_boot_sums) -> (sums fp64 [replicates + 1, n_seg, F], dropped
    int64 [3]); F = 7, or 10 with pred_b.  unit and seg: both int64 or both int32.  out: (sums, dropped) to write into."""
    n, dev = int(pred.numel()), pred.device
    if target.numel() != n or (pred_b is not None and pred_b.numel() != n):
        raise ValueError("boot_sums: pred, target and pred_b need the same length")
    if unit.dtype != seg.dtype or unit.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"boot_sums: unit and seg must both be int64 or both int32, got {unit.dtype} / {seg.dtype}")
    if unit.numel() != n or seg.numel() != n:
        raise ValueError(f"boot_sums: {unit.numel()} unit and {seg.numel()} segment indices for {n} pairs")
    n_seg, replicates = int(n_seg), int(replicates)
    F = n_fields(pred_b is not None)
    if out is None:
        out = (torch.empty(max(replicates, 0) + 1, max(n_seg, 0), F, dtype=torch.float64, device=dev),
               torch.empty(BOOT_DROP_KINDS, dtype=torch.int64, device=dev))
    sums, dropped = out
    if tuple(sums.shape) != (replicates + 1, n_seg, F):
        raise ValueError(f"boot_sums: sums must be [{replicates + 1}, {n_seg}, {F}], got {tuple(sums.shape)}")
    with_b = 1 if pred_b is not None else 0              # explicit: an empty pred_b is a null pointer
    nb = load().mmg_boot_sums_ws_bytes(n, n_seg, replicates, with_b)
    _call("mmg_boot_sums", pred, target, pred_b, with_b, ops._p(unit, unit.dtype, "unit"), ops._p(seg, seg.dtype, "seg"),
          unit.element_size(), n, int(n_units), n_seg, replicates, int(seed) & 0xFFFFFFFFFFFFFFFF, sums, dropped,
          ws=_ws(nb, dev))
    return sums, dropped


def boot_metrics(sums: torch.Tensor, out: Optional[torch.Tensor] = None):
    """sums [replicates + 1, n_seg, F] -> metrics fp64 [replicates + 1, n_seg + 1, M] (mmg_boot_metrics); row n_seg is all
    segments together; M = 4 (mae, rmse, r2, mape) or 12 for F = 10 (pred, pred_b, pred - pred_b)."""
    if sums.dim() != 3 or sums.shape[2] not in (BOOT_FIELDS, BOOT_FIELDS_B):
        raise ValueError(f"boot_metrics: sums must be [replicates + 1, n_seg, {BOOT_FIELDS} or {BOOT_FIELDS_B}]")
    with_b = sums.shape[2] == BOOT_FIELDS_B
    R1, n_seg = int(sums.shape[0]), int(sums.shape[1])
    if out is None:
        out = torch.empty(R1, n_seg + 1, n_metrics(with_b), dtype=torch.float64, device=sums.device)
    if tuple(out.shape) != (R1, n_seg + 1, n_metrics(with_b)):
        raise ValueError("boot_metrics: metrics must be [replicates + 1, n_seg + 1, M]")
    _call("mmg_boot_metrics", sums, n_seg, R1 - 1, 1 if with_b else 0, out)
    return out


def boot_summary(metrics: torch.Tensor, confidence: float = 0.95, out: Optional[torch.Tensor] = None):
    """metrics [replicates + 1, n_seg + 1, M] -> summary fp64 [n_seg + 1, M, 7]: estimate, mean, standard error, lower and
    upper percentile, number of finite replicates, share of them below zero (mmg_boot_summary)."""
    if metrics.dim() != 3 or metrics.shape[2] not in (BOOT_METRICS, BOOT_METRICS_B):
        raise ValueError(f"boot_summary: metrics must be [replicates + 1, n_seg + 1, {BOOT_METRICS} or {BOOT_METRICS_B}]")
    R1, rows, M = (int(x) for x in metrics.shape)
    if out is None:
        out = torch.empty(rows, M, BOOT_SUMMARY_FIELDS, dtype=torch.float64, device=metrics.device)
    if tuple(out.shape) != (rows, M, BOOT_SUMMARY_FIELDS):
        raise ValueError("boot_summary: summary must be [n_seg + 1, M, 7]")
    _call("mmg_boot_summary", metrics, rows - 1, R1 - 1, 1 if M == BOOT_METRICS_B else 0, float(confidence), out)
    return out
