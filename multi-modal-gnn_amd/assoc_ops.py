"""ctypes binding and typed entry points of libmmgnn_assoc.so (C ABI: include/mmgnn_assoc.h; csrc/assoc.hip): the
column statistics, the pairwise-complete moment planes and the correlation / covariance / Jaccard / lift epilogue of the
lab association tables, a library of its own beside libmmgnn.so.  The binding is a ``_lib.Binding`` derived from the
header, and every call goes through ``ops._call``.  The library is REQUIRED: there is no CPU or eager-PyTorch fallback
behind these calls (the numpy restatement of mmgnn/association.py serves numpy inputs and checks the kernels; it is
never a silent substitute for them).
"""
from __future__ import annotations

import torch

from . import ops

BINDING = ops.satellite("assoc", globals())    # LIB_PATH, HEADER_PATH, DEFINES, SIGNATURES, PARAMS, MMG_*, load, _call

AS_MAX_LABS = DEFINES["MMG_AS_MAX_LABS"]
AS_TILE = DEFINES["MMG_AS_TILE"]
AS_CHUNK = DEFINES["MMG_AS_CHUNK"]
AS_PLANES = DEFINES["MMG_AS_PLANES"]              # N, SX, SXX, SXY


def assoc_plan(n: int, n_labs: int):
    """The slab plan of assoc_moments (mmg_assoc_plan, a host function) -> (rows per slab, slabs)."""
    return ops.slab_plan(BINDING, "mmg_assoc_plan", n, n_labs)


def assoc_colstats(X: torch.Tensor):
    """Per lab the observed count (int64 [L]) and the fp64 mean of its observed values (0 for a lab nobody has), and
    the number of infinite cells (int64 [1]) (mmg_assoc_colstats), on the device."""
    px, n, L, ld = ops._lab_matrix(X, "assoc_colstats")
    dev = X.device
    count = torch.empty(max(L, 0), dtype=torch.int64, device=dev)
    mean = torch.empty(max(L, 0), dtype=torch.float64, device=dev)
    n_inf = torch.empty(1, dtype=torch.int64, device=dev)
    _call("mmg_assoc_colstats", px, n, L, ld, count, mean, n_inf,
          ws=ops._ws(load().mmg_assoc_colstats_ws_bytes(n, L), dev))
    return count, mean, n_inf


def assoc_moments(X: torch.Tensor, center: torch.Tensor):
    """The planes N, SX, SXX, SXY (fp64 [4, L, L]) of X about `center` (fp64 [L] on the device) (mmg_assoc_moments)."""
    px, n, L, ld = ops._lab_matrix(X, "assoc_moments")
    if center.dim() != 1 or center.numel() != L:
        raise ValueError(f"assoc_moments: center must hold {L} values, got {tuple(center.shape)}")
    if center.device != X.device:
        raise ValueError(f"assoc_moments: center is on {center.device}, X on {X.device}")
    out = torch.empty(AS_PLANES, max(L, 0), max(L, 0), dtype=torch.float64, device=X.device)
    _call("mmg_assoc_moments", px, n, L, ld, center, out, ws=ops._ws(load().mmg_assoc_moments_ws_bytes(n, L), X.device))
    return out


def assoc_finish(moments: torch.Tensor, count: torch.Tensor, n: int, min_periods: int = 1):
    """moments [4, L, L], count int64 [L] -> (r, cov, jaccard, lift), fp64 [L, L] each (mmg_assoc_finish)."""
    if moments.dim() != 3 or moments.shape[0] != AS_PLANES or moments.shape[1] != moments.shape[2]:
        raise ValueError(f"assoc_finish: moments must be [{AS_PLANES}, L, L], got {tuple(moments.shape)}")
    L = int(moments.shape[1])
    if count.numel() != L:
        raise ValueError(f"assoc_finish: count must hold {L} values, got {count.numel()}")
    out = [torch.empty(L, L, dtype=torch.float64, device=moments.device) for _ in range(4)]
    _call("mmg_assoc_finish", moments, count, L, int(n), int(min_periods), *out)
    return tuple(out)
