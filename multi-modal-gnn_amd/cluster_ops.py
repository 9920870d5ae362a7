"""ctypes binding and typed entry points of libmmgnn_cluster.so (C ABI: include/mmgnn_cluster.h; csrc/cluster.hip): k-means
and the cluster scores, a library of its own beside libmmgnn.so.  The binding is a ``_lib.Binding`` derived from the
header, and every call goes through ``ops._call``.  The library is REQUIRED: there is no CPU or eager-PyTorch fallback
behind these calls.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from ._lib import check

BINDING = ops.satellite("cluster", globals())    # LIB_PATH, HEADER_PATH, DEFINES, SIGNATURES, PARAMS, MMG_*, load, _call

KM_MAX_K = DEFINES["MMG_KM_MAX_K"]                  # csrc/cluster.hip: 1 <= k <= KM_MAX_K
KM_MAX_D = DEFINES["MMG_KM_MAX_D"]                  # the widest row
KM_ROW_TILE = DEFINES["MMG_KM_ROW_TILE"]            # rows of a workgroup's block, rows per LDS tile
KM_MAX_RANGES = DEFINES["MMG_KM_MAX_RANGES"]        # row ranges of the fixed-order sums
KM_MAX_GRID = DEFINES["MMG_KM_MAX_GRID"]            # workgroups of a launch: each walks work items in strides of the grid


def km_plan(n: int):
    """How the fixed-order sums and the assignment walk n rows (mmg_km_plan, host arithmetic) -> (row ranges, rows per
    range, workgroups of the assignment: fewer than row blocks = a workgroup takes several)."""
    import numpy as np
    out = np.zeros(3, np.int64)
    check(load().mmg_km_plan(int(n), out.ctypes.data), "mmg_km_plan")
    return int(out[0]), int(out[1]), int(out[2])


def km_sil_plan(n: int, nq: Optional[int] = None):
    """How mmg_km_silhouette walks n candidates and nq queries -> (candidate ranges, work items, workgroups)."""
    import numpy as np
    out = np.zeros(3, np.int64)
    check(load().mmg_km_sil_plan(int(n), int(n if nq is None else nq), out.ctypes.data), "mmg_km_sil_plan")
    return int(out[0]), int(out[1]), int(out[2])


def _centers(c: torch.Tensor, D: int, name: str) -> int:
    if c.dim() != 2 or int(c.shape[1]) != D or c.dtype != torch.float64 or not c.is_contiguous():
        raise ValueError(f"{name}: expected contiguous torch.float64 [k, {D}]")
    return int(c.shape[0])


def km_assign(x: torch.Tensor, centers: torch.Tensor, prev_labels: Optional[torch.Tensor] = None,
              labels: Optional[torch.Tensor] = None, min_s: Optional[torch.Tensor] = None,
              changed: Optional[torch.Tensor] = None):
    """label(i) = the centre with the smallest key (fp64 difference-form squared distance, centre index) of fp32 x [n, D]
    against fp64 centers [k, D] (mmg_km_assign) -> (labels int32 [n], min_s fp64 [n]).  changed (int64 [1]): the rows whose
    label differs from prev_labels (which may be `labels` itself; None: every row)."""
    px, n, D, ld = ops._rows_matrix(x, "x")
    k = _centers(centers, D, "centers")
    if labels is None:
        labels = torch.empty(n, dtype=torch.int32, device=x.device)
    if min_s is None:
        min_s = torch.empty(n, dtype=torch.float64, device=x.device)
    if labels.numel() != n or min_s.numel() != n or (prev_labels is not None and prev_labels.numel() != n):
        raise ValueError(f"km_assign: labels, min_s and prev_labels need {n} entries")
    _call("mmg_km_assign", px, n, D, ld, centers, k, prev_labels, labels, min_s, changed,
          ws=ops._ws(load().mmg_km_assign_ws_bytes(n, D, k), x.device))
    return labels, min_s


def km_label_dist(x: torch.Tensor, centers: torch.Tensor, labels: torch.Tensor):
    """s(i, labels(i)): every row's squared distance to its OWN centre (mmg_km_label_dist) -> fp64 [n]."""
    px, n, D, ld = ops._rows_matrix(x, "x")
    k = _centers(centers, D, "centers")
    if labels.numel() != n:
        raise ValueError(f"km_label_dist: labels needs {n} entries")
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    _call("mmg_km_label_dist", px, n, D, ld, centers, k, labels, out)
    return out


def km_update(x: torch.Tensor, labels: torch.Tensor, min_s: torch.Tensor, centers_old: torch.Tensor,
              centers_new: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
              changed: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
              reloc_rows: Optional[torch.Tensor] = None):
    """The centre update of one Lloyd iteration with the relocation of empty clusters (mmg_km_update) -> (centers_new
    fp64 [k, D] -- may be centers_old --, counts int32 [k], status fp64 [3] = (changed, shift, empty clusters))."""
    px, n, D, ld = ops._rows_matrix(x, "x")
    k = _centers(centers_old, D, "centers_old")
    if centers_new is None:
        centers_new = torch.empty_like(centers_old)
    elif _centers(centers_new, D, "centers_new") != k:
        raise ValueError(f"km_update: centers_new must be [{k}, {D}]")
    if counts is None:
        counts = torch.empty(k, dtype=torch.int32, device=x.device)
    if status is None:
        status = torch.empty(3, dtype=torch.float64, device=x.device)
    if labels.numel() != n or min_s.numel() != n or counts.numel() != k or status.numel() != 3:
        raise ValueError(f"km_update: labels and min_s need {n} entries, counts {k}, status 3")
    if reloc_rows is not None and reloc_rows.numel() != k:
        raise ValueError(f"km_update: reloc_rows needs {k} entries")
    _call("mmg_km_update", px, n, D, ld, labels, min_s, centers_old, k, centers_new, counts, changed, status, reloc_rows,
          ws=ops._ws(load().mmg_km_update_ws_bytes(n, D, k), x.device))
    return centers_new, counts, status


def km_colstats(x: torch.Tensor):
    """Column means (fp64 [D]) and the mean over the columns of their population variance (fp64 [1]) of fp32 x [n, D]
    (mmg_km_colstats), on the device."""
    px, n, D, ld = ops._rows_matrix(x, "x")
    mean = torch.empty(D, dtype=torch.float64, device=x.device)
    var = torch.empty(1, dtype=torch.float64, device=x.device)
    _call("mmg_km_colstats", px, n, D, ld, mean, var, ws=ops._ws(load().mmg_km_colstats_ws_bytes(n, D), x.device))
    return mean, var


def km_scores(labels: torch.Tensor, min_s: torch.Tensor, k: int):
    """(inertia fp64 [1] = sum min_s, sdist fp64 [k] = per cluster the sum of sqrt(min_s), counts int32 [k])
    (mmg_km_scores): fixed-order sums."""
    n, k = int(labels.numel()), int(k)
    if min_s.numel() != n:
        raise ValueError(f"km_scores: min_s needs {n} entries")
    inertia = torch.empty(1, dtype=torch.float64, device=labels.device)
    sdist = torch.empty(k, dtype=torch.float64, device=labels.device)
    counts = torch.empty(k, dtype=torch.int32, device=labels.device)
    _call("mmg_km_scores", labels, min_s, n, k, inertia, sdist, counts, ws=ops._ws(load().mmg_km_scores_ws_bytes(n, k), labels.device))
    return inertia, sdist, counts


def km_silhouette(x: torch.Tensor, labels: torch.Tensor, counts: torch.Tensor, queries: Optional[torch.Tensor] = None,
                  want_mean: bool = True):
    """Silhouette coefficients of the rows `queries` (int32 [nq]; None: all rows) of fp32 x [n, D] under labels int32 [n]
    with counts int32 [k] rows per label (mmg_km_silhouette) -> (sil fp64 [nq], mean fp64 [1] or None)."""
    px, n, D, ld = ops._rows_matrix(x, "x")
    k = int(counts.numel())
    if labels.numel() != n:
        raise ValueError(f"km_silhouette: labels needs {n} entries")
    nq = n if queries is None else int(queries.numel())
    sil = torch.empty(nq, dtype=torch.float64, device=x.device)
    mean = torch.empty(1, dtype=torch.float64, device=x.device) if want_mean else None
    _call("mmg_km_silhouette", px, n, D, ld, labels, counts, k, queries, nq, sil, mean,
          ws=ops._ws(load().mmg_km_silhouette_ws_bytes(n, D, nq, k), x.device))
    return sil, mean
