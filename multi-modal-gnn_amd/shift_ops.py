"""ctypes binding and typed entry points of libmmgnn_shift.so (C ABI: include/mmgnn_shift.h; csrc/shift.hip): the
permutation thresholds, the per-lab two-sample statistics of every replicate, their finish and the p-values, a library of
its own beside libmmgnn.so.  The binding is a ``_lib.Binding`` derived from the header, and every call goes through
``ops._call``.  The library is REQUIRED: there is no CPU or eager-PyTorch fallback behind these calls (the numpy
restatement of mmgnn/shift.py serves numpy inputs and checks the kernels; it is never a silent substitute for them).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops

BINDING = ops.satellite("shift", globals())    # LIB_PATH, HEADER_PATH, DEFINES, SIGNATURES, PARAMS, MMG_*, load, _call

SHIFT_SITE = DEFINES["MMG_SHIFT_SITE"]
SHIFT_MAX_REPLICATES = DEFINES["MMG_SHIFT_MAX_REPLICATES"]
SHIFT_MAX_SEG = DEFINES["MMG_SHIFT_MAX_SEG"]
SHIFT_CHUNK = DEFINES["MMG_SHIFT_CHUNK"]                  # C: sorted pairs per chunk
SHIFT_RB = DEFINES["MMG_SHIFT_RB"]                        # RB: replicates per workgroup
SHIFT_DROP_KINDS = DEFINES["MMG_SHIFT_DROP_KINDS"]        # lab, unit out of range; NaN or infinite value; unit in no cohort
SHIFT_COUNTS = DEFINES["MMG_SHIFT_COUNTS"]                # U, U_A, status
SHIFT_OK = DEFINES["MMG_SHIFT_OK"]
SHIFT_BAD_COHORTS = DEFINES["MMG_SHIFT_BAD_COHORTS"]
SHIFT_INT_FIELDS = DEFINES["MMG_SHIFT_INT_FIELDS"]
SHIFT_SUM_FIELDS = DEFINES["MMG_SHIFT_SUM_FIELDS"]
SHIFT_STAT_FIELDS = DEFINES["MMG_SHIFT_STAT_FIELDS"]
SHIFT_SUMMARY_FIELDS = DEFINES["MMG_SHIFT_SUMMARY_FIELDS"]


def _seed(seed) -> int:
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def shift_thresholds(group: torch.Tensor, replicates: int, seed: int = 0, out=None):
    """group uint8 [n_units] -> (T int64 [replicates + 1] holding the uint64 thresholds bit for bit, cohort int64 [3]:
    U, U_A, status) (mmg_shift_thresholds).  The status is NOT read here: no call of this module synchronises."""
    replicates = int(replicates)
    if out is None:
        out = (torch.empty(max(replicates, 0) + 1, dtype=torch.int64, device=group.device),
               torch.empty(SHIFT_COUNTS, dtype=torch.int64, device=group.device))
    T, cohort = out
    if T.numel() != replicates + 1 or cohort.numel() != SHIFT_COUNTS:
        raise ValueError(f"shift_thresholds: T must be [{replicates + 1}] and cohort [{SHIFT_COUNTS}]")
    _call("mmg_shift_thresholds", group, int(group.numel()), replicates, _seed(seed), T, cohort)
    return T, cohort


def shift_stats(value: torch.Tensor, seg: torch.Tensor, unit: torch.Tensor, group: torch.Tensor, n_seg: int,
                T: torch.Tensor, seed: int = 0, out=None):
    """The integer and fp64 tables of every replicate (mmg_shift_stats) -> (counts int64 [R + 1, n_seg, 4], sums fp64
    [R + 1, n_seg, 5], dropped int64 [4]); R + 1 = len(T).  seg and unit: both int64 or both int32.  out: the three to
    write into."""
    n, dev = int(value.numel()), value.device
    if unit.dtype != seg.dtype or unit.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"shift_stats: seg and unit must both be int64 or both int32, got {seg.dtype} / {unit.dtype}")
    if unit.numel() != n or seg.numel() != n:
        raise ValueError(f"shift_stats: {seg.numel()} lab and {unit.numel()} unit indices for {n} pairs")
    n_seg, R1 = int(n_seg), int(T.numel())
    if out is None:
        out = (torch.empty(R1, max(n_seg, 0), SHIFT_INT_FIELDS, dtype=torch.int64, device=dev),
               torch.empty(R1, max(n_seg, 0), SHIFT_SUM_FIELDS, dtype=torch.float64, device=dev),
               torch.empty(SHIFT_DROP_KINDS, dtype=torch.int64, device=dev))
    counts, sums, dropped = out
    if tuple(counts.shape) != (R1, n_seg, SHIFT_INT_FIELDS) or tuple(sums.shape) != (R1, n_seg, SHIFT_SUM_FIELDS):
        raise ValueError(f"shift_stats: counts must be [{R1}, {n_seg}, {SHIFT_INT_FIELDS}] and sums "
                         f"[{R1}, {n_seg}, {SHIFT_SUM_FIELDS}]")
    nb = load().mmg_shift_stats_ws_bytes(n, n_seg, R1 - 1)
    _call("mmg_shift_stats", value, ops._p(seg, seg.dtype, "seg"), ops._p(unit, unit.dtype, "unit"), unit.element_size(), n,
          n_seg, group, int(group.numel()), R1 - 1, _seed(seed), T, counts, sums, dropped, ws=ops._ws(nb, dev))
    return counts, sums, dropped


def shift_finish(counts: torch.Tensor, sums: torch.Tensor, cohort: torch.Tensor, out: Optional[torch.Tensor] = None):
    """counts, sums, cohort -> stats fp64 [R + 1, n_seg + 1, 6]: D, D_signed, W1, smd, z, cov; row n_seg holds the
    maximum of z over the labs in field 4 (mmg_shift_finish)."""
    if counts.dim() != 3 or counts.shape[2] != SHIFT_INT_FIELDS or tuple(sums.shape) != (*counts.shape[:2], SHIFT_SUM_FIELDS):
        raise ValueError(f"shift_finish: counts [R + 1, n_seg, {SHIFT_INT_FIELDS}] and sums [R + 1, n_seg, {SHIFT_SUM_FIELDS}]")
    R1, n_seg = int(counts.shape[0]), int(counts.shape[1])
    if out is None:
        out = torch.empty(R1, n_seg + 1, SHIFT_STAT_FIELDS, dtype=torch.float64, device=counts.device)
    if tuple(out.shape) != (R1, n_seg + 1, SHIFT_STAT_FIELDS):
        raise ValueError(f"shift_finish: stats must be [R + 1, n_seg + 1, {SHIFT_STAT_FIELDS}]")
    _call("mmg_shift_finish", counts, sums, cohort, n_seg, R1 - 1, out)
    return out


def shift_summary(stats: torch.Tensor, out: Optional[torch.Tensor] = None):
    """stats [R + 1, n_seg + 1, 6] -> summary fp64 [n_seg + 1, 7]: the permutation p-values of D, W1, |smd|, |cov|, the
    maxT-adjusted p-value, and the counts behind the first and the last (mmg_shift_summary)."""
    if stats.dim() != 3 or stats.shape[2] != SHIFT_STAT_FIELDS:
        raise ValueError(f"shift_summary: stats must be [R + 1, n_seg + 1, {SHIFT_STAT_FIELDS}]")
    R1, rows = int(stats.shape[0]), int(stats.shape[1])
    if out is None:
        out = torch.empty(rows, SHIFT_SUMMARY_FIELDS, dtype=torch.float64, device=stats.device)
    if tuple(out.shape) != (rows, SHIFT_SUMMARY_FIELDS):
        raise ValueError(f"shift_summary: summary must be [n_seg + 1, {SHIFT_SUMMARY_FIELDS}]")
    _call("mmg_shift_summary", stats, rows - 1, R1 - 1, out)
    return out
