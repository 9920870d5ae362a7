"""ctypes binding and typed entry points of libmmgnn_conformal.so (C ABI: include/mmgnn_conformal.h; csrc/conformal.hip):
segmented order statistics, the conformal table, the interval epilogues and their coverage counts, a library of its own
beside libmmgnn.so.  The binding is a ``_lib.Binding`` derived from the header, and every call goes through
``ops._call``.  The library is REQUIRED: there is no CPU or eager-PyTorch fallback behind these calls (the numpy
restatement of mmgnn/conformal.py serves numpy inputs and checks the kernels; it is never a silent substitute for them).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops

BINDING = ops.satellite("conformal", globals())    # LIB_PATH, HEADER_PATH, DEFINES, SIGNATURES, PARAMS, MMG_*, load, _call

CF_SIGNED = DEFINES["MMG_CF_SIGNED"]
CF_ABSOLUTE = DEFINES["MMG_CF_ABSOLUTE"]
CF_MAX_LABS = DEFINES["MMG_CF_MAX_LABS"]
CF_MAX_BINS = DEFINES["MMG_CF_MAX_BINS"]
CF_MAX_CELLS = DEFINES["MMG_CF_MAX_CELLS"]
CF_DROP_KINDS = DEFINES["MMG_CF_DROP_KINDS"]      # lab out of range, patient out of range, degree in no bin, NaN key
CF_COV_FIELDS = DEFINES["MMG_CF_COV_FIELDS"]      # n, covered, below, above, infinite, dropped
MODES = {"signed": CF_SIGNED, "absolute": CF_ABSOLUTE}


def seg_order_stats(keys: torch.Tensor, seg: torch.Tensor, n_seg: int, alpha: float, mode: str = "signed",
                    min_count: int = 0):
    """Per segment the conformal order statistics of fp32 keys [n] under int32 segment ids [n] in [0, n_seg] (n_seg and
    NaN keys: ignored) (mmg_seg_order_stats) -> (count int32, q_lo, q_hi, shift fp32, usable int32), each [n_seg]."""
    n, dev = int(keys.numel()), keys.device
    if seg.numel() != n:
        raise ValueError(f"seg_order_stats: {seg.numel()} segment ids for {n} keys")
    n_seg = int(n_seg)
    count = torch.empty(max(n_seg, 0), dtype=torch.int32, device=dev)
    usable = torch.empty_like(count)
    q_lo, q_hi, shift = (torch.empty(max(n_seg, 0), dtype=torch.float32, device=dev) for _ in range(3))
    _call("mmg_seg_order_stats", keys, seg, n, n_seg, float(alpha), MODES[mode], int(min_count), count, q_lo, q_hi, shift,
          usable, ws=ops._ws(load().mmg_seg_order_stats_ws_bytes(n, n_seg), dev))
    return count, q_lo, q_hi, shift, usable


def cf_fit(pred: torch.Tensor, target: torch.Tensor, patient: torch.Tensor, lab: torch.Tensor, n_labs: int,
           deg: torch.Tensor, bin_edges, alpha: float, mode: str = "signed", min_count: int = 0):
    """The conformal table of the calibration pairs (mmg_cf_fit) -> (table fp32 [3, n_cells]: q_lo, q_hi, shift; level
    int32 [n_cells]; n_used int32 [n_cells]; dropped int64 [4]), on the device."""
    n, dev = int(pred.numel()), pred.device
    if target.numel() != n:
        raise ValueError("cf_fit: pred and target need the same length")
    pp, pl, ib = ops._index_pair(patient, lab, n, "cf_fit")
    ed, n_bins = ops._edges(bin_edges)
    n_labs = int(n_labs)
    n_cells = max(n_labs * n_bins, 0)
    table = torch.empty(3, n_cells, dtype=torch.float32, device=dev)
    level = torch.empty(n_cells, dtype=torch.int32, device=dev)
    n_used = torch.empty(n_cells, dtype=torch.int32, device=dev)
    dropped = torch.empty(CF_DROP_KINDS, dtype=torch.int64, device=dev)
    _call("mmg_cf_fit", pred, target, pp, pl, ib, n, n_labs, deg, int(deg.numel()), ed, n_bins, float(alpha), MODES[mode],
          int(min_count), table, level, n_used, dropped, ws=ops._ws(load().mmg_cf_fit_ws_bytes(n, n_labs, n_bins), dev))
    return table, level, n_used, dropped


def _check_table(table: torch.Tensor, n_labs: int, n_bins: int, what: str):
    if table.dim() != 2 or tuple(table.shape) != (3, n_labs * n_bins):
        raise ValueError(f"{what}: table must be [3, {n_labs * n_bins}], got {tuple(table.shape)}")


def cf_apply_pairs(pred: torch.Tensor, patient: torch.Tensor, lab: torch.Tensor, n_labs: int, deg: torch.Tensor, bin_edges,
                   table: torch.Tensor, use_shift: bool = False):
    """(point, lower, upper) fp32 [n] of the pairs under the table (mmg_cf_apply_pairs)."""
    n, dev = int(pred.numel()), pred.device
    pp, pl, ib = ops._index_pair(patient, lab, n, "cf_apply_pairs")
    ed, n_bins = ops._edges(bin_edges)
    _check_table(table, int(n_labs), n_bins, "cf_apply_pairs")
    point, lower, upper = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
    _call("mmg_cf_apply_pairs", pred, pp, pl, ib, n, int(n_labs), deg, int(deg.numel()), ed, n_bins, table,
          1 if use_shift else 0, point, lower, upper)
    return point, lower, upper


def cf_apply_matrix(pred: torch.Tensor, rows: Optional[torch.Tensor], deg: torch.Tensor, bin_edges, table: torch.Tensor,
                    use_shift: bool = False, out=None):
    """(point, lower, upper) fp32 [n_rows, n_labs] of a dense prediction matrix (rows may be strided) under the table
    (mmg_cf_apply_matrix).  rows: int64 / int32 [n_rows] patient index of every row, None: row i is patient i.  out: three
    [n_rows, n_labs] fp32 views with unit column stride and ONE common row stride."""
    px, n_rows, n_labs, ld = ops._rows_matrix(pred, "pred")
    ed, n_bins = ops._edges(bin_edges)
    _check_table(table, n_labs, n_bins, "cf_apply_matrix")
    pr, ib = None, 8
    if rows is not None:
        if rows.dtype not in (torch.int64, torch.int32) or rows.numel() != n_rows:
            raise ValueError(f"cf_apply_matrix: rows must be {n_rows} int64 or int32 patient indices")
        pr, ib = ops._p(rows, rows.dtype, "rows"), rows.element_size()
    if out is None:
        out = tuple(torch.empty(n_rows, n_labs, dtype=torch.float32, device=pred.device) for _ in range(3))
    ptrs, lds = [], set()
    for o, name in zip(out, ("point", "lower", "upper")):
        po, r, c, ldo = ops._rows_matrix(o, name)
        if (r, c) != (n_rows, n_labs):
            raise ValueError(f"cf_apply_matrix: {name} must be [{n_rows}, {n_labs}]")
        ptrs.append(po)
        lds.add(ldo)
    if len(lds) != 1:
        raise ValueError("cf_apply_matrix: the three outputs need one common row stride")
    _call("mmg_cf_apply_matrix", px, n_rows, n_labs, ld, pr, ib, deg, int(deg.numel()), ed, n_bins, table,
          1 if use_shift else 0, ptrs[0], ptrs[1], ptrs[2], lds.pop())
    return tuple(out)


def cf_coverage(pred: torch.Tensor, target: torch.Tensor, patient: torch.Tensor, lab: torch.Tensor, n_labs: int,
                deg: torch.Tensor, bin_edges, table: torch.Tensor):
    """Per cell the coverage counts of the evaluation pairs under the table (mmg_cf_coverage) -> (counts int64
    [n_cells + 1, 6], width fp64 [n_cells + 1]); the last row: the pairs without a cell."""
    n, dev = int(pred.numel()), pred.device
    if target.numel() != n:
        raise ValueError("cf_coverage: pred and target need the same length")
    pp, pl, ib = ops._index_pair(patient, lab, n, "cf_coverage")
    ed, n_bins = ops._edges(bin_edges)
    n_labs = int(n_labs)
    _check_table(table, n_labs, n_bins, "cf_coverage")
    n_cells = n_labs * n_bins
    counts = torch.empty(n_cells + 1, CF_COV_FIELDS, dtype=torch.int64, device=dev)
    width = torch.empty(n_cells + 1, dtype=torch.float64, device=dev)
    _call("mmg_cf_coverage", pred, target, pp, pl, ib, n, n_labs, deg, int(deg.numel()), ed, n_bins, table, counts, width,
          ws=ops._ws(load().mmg_cf_coverage_ws_bytes(n, n_labs, n_bins), dev))
    return counts, width
