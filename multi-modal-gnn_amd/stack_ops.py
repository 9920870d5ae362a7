"""ctypes binding and typed entry points of libmmgnn_stack.so (C ABI: include/mmgnn_stack.h; csrc/stack.hip): the
normal-equation sums, the per-cell ridge solve, the two apply epilogues and the before/after scores of the stacked
recalibration, a library of its own beside libmmgnn.so.  The binding is a ``_lib.Binding`` derived from the header, and
every call goes through ``ops._call``.  The library is REQUIRED: there is no CPU or eager-PyTorch fallback behind these
calls (the numpy restatement of mmgnn/stacking.py serves numpy inputs and checks the kernels; it is never a silent
substitute for them).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import ops

BINDING = ops.satellite("stack", globals())    # LIB_PATH, HEADER_PATH, DEFINES, SIGNATURES, PARAMS, MMG_*, load, _call

ST_SITE = DEFINES["MMG_ST_SITE"]
ST_MAX_FEATURES = DEFINES["MMG_ST_MAX_FEATURES"]
ST_MAX_FOLDS = DEFINES["MMG_ST_MAX_FOLDS"]
ST_MAX_LABS = DEFINES["MMG_ST_MAX_LABS"]
ST_MAX_BINS = DEFINES["MMG_ST_MAX_BINS"]
ST_MAX_CELLS = DEFINES["MMG_ST_MAX_CELLS"]
ST_CHUNK = DEFINES["MMG_ST_CHUNK"]
ST_DROP_KINDS = DEFINES["MMG_ST_DROP_KINDS"]      # lab out of range, patient out of range, degree in no bin, a NaN value
ST_SCORE_FIELDS = DEFINES["MMG_ST_SCORE_FIELDS"]  # n, sum |t - raw|, sum (t - raw)^2, sum |t - stacked|, sum (t - stacked)^2
ST_PIVOT_REL = float(f"1e{DEFINES['MMG_ST_PIVOT_REL_LOG10']}")


def _feature_list(feats: Sequence[torch.Tensor], what: str):
    """K fp32 device vectors of one length -> (host array of their K device pointers, K, n, device)."""
    feats = list(feats)
    if not 1 <= len(feats) <= ST_MAX_FEATURES:
        raise ValueError(f"{what}: {len(feats)} features outside [1, {ST_MAX_FEATURES}]")
    n, dev = int(feats[0].numel()), feats[0].device
    ptrs = []
    for k, f in enumerate(feats):
        if f.dim() != 1 or f.numel() != n:
            raise ValueError(f"{what}: feature {k} must be a vector of {n} values, got {tuple(f.shape)}")
        if f.device != dev:
            raise ValueError(f"{what}: feature {k} is on {f.device}, the features before it on {dev}")
        ptrs.append(ops._p(f, torch.float32, f"feature {k}").value or 0)
    return (C.c_void_p * len(ptrs))(*ptrs), len(ptrs), n, dev


def n_fields(n_features: int) -> int:
    """F: the sums per (fold, cell)."""
    k = int(n_features)
    return (k + 1) * (k + 2) // 2 + k + 2


def folds_out(folds: int) -> int:
    """Rows of the coefficient table: one per left-out fold and one for all pairs (folds = 1: that one alone)."""
    return int(folds) + 1 if int(folds) > 1 else 1


def stack_sums(feats, target: torch.Tensor, patient: torch.Tensor, lab: torch.Tensor, n_labs: int, deg: torch.Tensor,
               bin_edges, folds: int = 1, seed: int = 0):
    """The normal-equation sums per (fold, cell) (mmg_stack_sums) -> (sums fp64 [folds, n_cells, F], dropped int64 [4]),
    on the device."""
    fp, K, n, dev = _feature_list(feats, "stack_sums")
    if target.numel() != n:
        raise ValueError("stack_sums: features and target need the same length")
    pp, pl, ib = ops._index_pair(patient, lab, n, "stack_sums")
    ed, n_bins = ops._edges(bin_edges)
    n_labs, folds = int(n_labs), int(folds)
    sums = torch.empty(max(folds, 0), max(n_labs * n_bins, 0), n_fields(K), dtype=torch.float64, device=dev)
    dropped = torch.empty(ST_DROP_KINDS, dtype=torch.int64, device=dev)
    _call("mmg_stack_sums", fp, K, target, pp, pl, ib, n, n_labs, deg, int(deg.numel()), ed, n_bins, folds,
          int(seed) & 0xFFFFFFFFFFFFFFFF, sums, dropped,
          ws=ops._ws(load().mmg_stack_sums_ws_bytes(n, n_labs, n_bins, K, folds), dev))
    return sums, dropped


def stack_solve(sums: torch.Tensor, n_labs: int, n_bins: int, n_features: int, ridge: float, min_count: int):
    """sums [folds, n_cells, F] -> (coef fp64 [folds_out, n_cells, K + 1], level int32, n_used int32 [folds_out, n_cells])
    (mmg_stack_solve)."""
    K, n_labs, n_bins = int(n_features), int(n_labs), int(n_bins)
    if sums.dim() != 3 or tuple(sums.shape[1:]) != (n_labs * n_bins, n_fields(K)):
        raise ValueError(f"stack_solve: sums must be [folds, {n_labs * n_bins}, {n_fields(K)}], got {tuple(sums.shape)}")
    folds, dev = int(sums.shape[0]), sums.device
    fo = folds_out(folds)
    coef = torch.empty(fo, n_labs * n_bins, K + 1, dtype=torch.float64, device=dev)
    level = torch.empty(fo, n_labs * n_bins, dtype=torch.int32, device=dev)
    n_used = torch.empty_like(level)
    _call("mmg_stack_solve", sums, n_labs, n_bins, K, folds, float(ridge), int(min_count), coef, level, n_used,
          ws=ops._ws(load().mmg_stack_solve_ws_bytes(n_labs, n_bins, K, folds), dev))
    return coef, level, n_used


def _check_coef(coef: torch.Tensor, n_cells: int, K: int, what: str) -> int:
    """-> folds of a coefficient table [folds_out, n_cells, K + 1]."""
    if coef.dim() != 3 or tuple(coef.shape[1:]) != (n_cells, K + 1) or coef.shape[0] < 1 or coef.shape[0] == 2:
        raise ValueError(f"{what}: coef must be [folds_out, {n_cells}, {K + 1}], got {tuple(coef.shape)}")
    return int(coef.shape[0]) - 1 if coef.shape[0] > 1 else 1


def stack_apply_pairs(feats, patient: torch.Tensor, lab: torch.Tensor, n_labs: int, deg: torch.Tensor, bin_edges,
                      coef: torch.Tensor, seed: int = 0, cross: bool = False):
    """The stacked prediction fp32 [n] of the pairs (mmg_stack_apply_pairs); cross: every pair under the coefficients
    fitted without its own patient's fold."""
    fp, K, n, dev = _feature_list(feats, "stack_apply_pairs")
    pp, pl, ib = ops._index_pair(patient, lab, n, "stack_apply_pairs")
    ed, n_bins = ops._edges(bin_edges)
    folds = _check_coef(coef, int(n_labs) * n_bins, K, "stack_apply_pairs")
    out = torch.empty(n, dtype=torch.float32, device=dev)
    _call("mmg_stack_apply_pairs", fp, K, pp, pl, ib, n, int(n_labs), deg, int(deg.numel()), ed, n_bins, coef, folds,
          int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if cross else 0, out)
    return out


def stack_apply_matrix(feats, rows: Optional[torch.Tensor], deg: torch.Tensor, bin_edges, coef: torch.Tensor, seed: int = 0,
                       cross: bool = False, out: Optional[torch.Tensor] = None):
    """The stacked prediction fp32 [n_rows, n_labs] of dense features (mmg_stack_apply_matrix).  feats[0] is a matrix
    [n_rows, n_labs] (rows may be strided); every other feature is such a matrix or a vector [n_labs] broadcast over the
    rows.  rows: int64 / int32 [n_rows] patient index of every row, None: row i is patient i.  out: an fp32 [n_rows,
    n_labs] view with unit column stride."""
    feats = list(feats)
    if not 1 <= len(feats) <= ST_MAX_FEATURES:
        raise ValueError(f"stack_apply_matrix: {len(feats)} features outside [1, {ST_MAX_FEATURES}]")
    p0, n_rows, n_labs, ld0 = ops._rows_matrix(feats[0], "feature 0")
    dev = feats[0].device
    ptrs, lds = [p0.value or 0], [ld0]
    for k, f in enumerate(feats[1:], 1):
        if f.device != dev:
            raise ValueError(f"stack_apply_matrix: feature {k} is on {f.device}, feature 0 on {dev}")
        if f.dim() == 1:
            if f.numel() != n_labs:
                raise ValueError(f"stack_apply_matrix: the broadcast feature {k} needs {n_labs} values, got {f.numel()}")
            ptrs.append(ops._p(f, torch.float32, f"feature {k}").value or 0)
            lds.append(0)
        else:
            pk, r, c, ldk = ops._rows_matrix(f, f"feature {k}")
            if (r, c) != (n_rows, n_labs):
                raise ValueError(f"stack_apply_matrix: feature {k} must be [{n_rows}, {n_labs}] or [{n_labs}]")
            ptrs.append(pk.value or 0)
            lds.append(ldk)
    K = len(ptrs)
    ed, n_bins = ops._edges(bin_edges)
    folds = _check_coef(coef, n_labs * n_bins, K, "stack_apply_matrix")
    pr, ib = None, 8
    if rows is not None:
        if rows.dtype not in (torch.int64, torch.int32) or rows.numel() != n_rows:
            raise ValueError(f"stack_apply_matrix: rows must be {n_rows} int64 or int32 patient indices")
        pr, ib = ops._p(rows, rows.dtype, "rows"), rows.element_size()
    if out is None:
        out = torch.empty(n_rows, n_labs, dtype=torch.float32, device=dev)
    po, r, c, ldo = ops._rows_matrix(out, "out")
    if (r, c) != (n_rows, n_labs):
        raise ValueError(f"stack_apply_matrix: out must be [{n_rows}, {n_labs}]")
    _call("mmg_stack_apply_matrix", (C.c_void_p * K)(*ptrs), (C.c_int64 * K)(*lds), K, n_rows, n_labs, pr, ib, deg,
          int(deg.numel()), ed, n_bins, coef, folds, int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if cross else 0, po, ldo)
    return out


def stack_scores(raw: torch.Tensor, stacked: torch.Tensor, target: torch.Tensor, patient: torch.Tensor, lab: torch.Tensor,
                 n_labs: int, deg: torch.Tensor, bin_edges):
    """Before / after error sums per cell, per lab and overall (mmg_stack_scores) -> (scores fp64 [n_cells + n_labs + 1,
    5], dropped int64 [4])."""
    n, dev = int(raw.numel()), raw.device
    if stacked.numel() != n or target.numel() != n:
        raise ValueError("stack_scores: raw, stacked and target need the same length")
    pp, pl, ib = ops._index_pair(patient, lab, n, "stack_scores")
    ed, n_bins = ops._edges(bin_edges)
    n_labs = int(n_labs)
    scores = torch.empty(max(n_labs * n_bins + n_labs + 1, 1), ST_SCORE_FIELDS, dtype=torch.float64, device=dev)
    dropped = torch.empty(ST_DROP_KINDS, dtype=torch.int64, device=dev)
    _call("mmg_stack_scores", raw, stacked, target, pp, pl, ib, n, n_labs, deg, int(deg.numel()), ed, n_bins, scores,
          dropped, ws=ops._ws(load().mmg_stack_scores_ws_bytes(n, n_labs, n_bins), dev))
    return scores, dropped
