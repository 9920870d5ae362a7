"""ctypes binding and typed entry points of libmmgnn_boot.so (C ABI: include/mmgnn_boot.h; csrc/boot.hip): the weighted
segment sums of the patient-cluster bootstrap, the metrics of every replicate and their summary, a library of its own
beside libmmgnn.so.  The binding is a ``_lib.Binding`` derived from the header, and every call goes through
``ops._call``.  The library is REQUIRED: there is no CPU or eager-PyTorch fallback behind these calls (the numpy
restatement of mmgnn/bootstrap.py serves numpy inputs and checks the kernels; it is never a silent substitute for them).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops

BINDING = ops.satellite("boot", globals())    # LIB_PATH, HEADER_PATH, DEFINES, SIGNATURES, PARAMS, MMG_*, load, _call

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
          ws=ops._ws(nb, dev))
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
