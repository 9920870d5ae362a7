"""ctypes binding and typed entry points of libmmgnn_nn.so (C ABI: include/mmgnn_nn.h; csrc/nn.hip): the embedding
neighbour kernels, a library of its own beside libmmgnn.so.  The binding is a ``_lib.Binding`` derived from the header,
and every call goes through ``ops._call``: a tensor handed to a scalar pointer is checked under the header's dtype and
name, ws / ws_bytes / stream are filled in there.  The library is REQUIRED: there is no CPU or eager-PyTorch fallback
behind these calls.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from ._lib import check

BINDING = ops.satellite("nn", globals())    # LIB_PATH, HEADER_PATH, DEFINES, SIGNATURES, PARAMS, MMG_*, load, _call

NN_MAX_K = DEFINES["MMG_NN_MAX_K"]                  # csrc/nn.hip: 1 <= k <= NN_MAX_K
NN_QUERY_BLOCK = DEFINES["MMG_NN_QUERY_BLOCK"]      # query rows of a workgroup
NN_TILE = DEFINES["MMG_NN_TILE"]                    # candidate rows per LDS tile
NN_MAX_GRID = DEFINES["MMG_NN_MAX_GRID"]            # workgroups of a launch: each walks work items in strides of the grid
NN_MAX_D = DEFINES["MMG_NN_MAX_D"]                  # the widest row


def nn_plan(n: int, nq: Optional[int] = None):
    """How mmg_nn_search walks n candidates and nq queries (mmg_nn_plan, host arithmetic) -> (candidate ranges, work
    items = query blocks x ranges, workgroups launched): more items than workgroups = a workgroup takes several; more
    than one range = the merge kernel runs."""
    import numpy as np
    out = np.zeros(3, np.int64)
    check(load().mmg_nn_plan(int(n), int(n if nq is None else nq), out.ctypes.data), "mmg_nn_plan")
    return int(out[0]), int(out[1]), int(out[2])


def _nn_out(t, n, k, dtype, device, name):
    """The [n, k] output of a neighbour call (unit column stride; the rows may be padded) -> (tensor, row stride)."""
    if t is None:
        t = torch.empty(n, k, dtype=dtype, device=device)
    if t.dim() != 2 or tuple(t.shape) != (n, k) or t.dtype != dtype or (k > 1 and t.stride(1) != 1):
        raise ValueError(f"{name}: expected {dtype} [{n}, {k}] with unit column stride")
    return t, (int(t.stride(0)) if n > 1 else max(int(t.stride(0)), k))


def nn_search(x: torch.Tensor, k: int, queries: Optional[torch.Tensor] = None, dist_out: Optional[torch.Tensor] = None,
              idx_out: Optional[torch.Tensor] = None):
    """The k nearest rows of fp32 x [n, D] for every query (mmg_nn_search): keys (fp64 difference-form squared distance,
    row index) in ascending order -> (distances fp32 [nq, k] = the fp64 root rounded once, indices int64 [nq, k]).
    queries None: self mode, every row of x queries the others (row q itself is skipped)."""
    px, n, D, ld = ops._rows_matrix(x, "x")
    if queries is None:
        pq, nq, ld_q = None, n, 0
    else:
        pq, nq, Dq, ld_q = ops._rows_matrix(queries, "queries")
        if Dq != D:
            raise ValueError(f"nn_search: queries have {Dq} columns, x has {D}")
        if queries.device != x.device:
            raise ValueError(f"nn_search: queries are on {queries.device}, x on {x.device}")
    k = int(k)
    dist_out, ld_d = _nn_out(dist_out, nq, k, torch.float32, x.device, "dist_out")
    idx_out, ld_i = _nn_out(idx_out, nq, k, torch.int64, x.device, "idx_out")
    _call("mmg_nn_search", px, n, D, ld, pq, nq, ld_q, k, ops._p(dist_out, torch.float32, "dist_out", contiguous=False),
          ld_d, ops._p(idx_out, torch.int64, "idx_out", contiguous=False), ld_i,
          ws=ops._ws(load().mmg_nn_search_ws_bytes(n, D, nq, k), x.device))
    return dist_out, idx_out


def nn_rank(x: torch.Tensor, nbr: torch.Tensor, want_rank: bool = True, want_penalty: bool = True,
            rank_out: Optional[torch.Tensor] = None):
    """Where the rows nbr [n, k] (int64) stand in each row's full neighbour order over fp32 x [n, D] (mmg_nn_rank) ->
    (rank int32 [n, k]: 1-based, 0 for an entry that is out of range or the row itself -- or None; penalty int64 [1] =
    sum max(0, rank - k), the numerator of sklearn's trustworthiness -- or None)."""
    px, n, D, ld = ops._rows_matrix(x, "x")
    if nbr.dim() != 2 or int(nbr.shape[0]) != n or (nbr.shape[1] > 1 and nbr.stride(1) != 1):
        raise ValueError(f"nn_rank: nbr must be [{n}, k] with unit column stride, got {tuple(nbr.shape)}")
    if nbr.device != x.device:
        raise ValueError(f"nn_rank: nbr is on {nbr.device}, x on {x.device}")
    k = int(nbr.shape[1])
    ld_n = int(nbr.stride(0)) if n > 1 else max(int(nbr.stride(0)), k)
    rank, ld_r = (None, 0)
    if want_rank or rank_out is not None:
        rank, ld_r = _nn_out(rank_out, n, k, torch.int32, x.device, "rank_out")
    penalty = torch.empty(1, dtype=torch.int64, device=x.device) if want_penalty else None
    _call("mmg_nn_rank", px, n, D, ld, ops._p(nbr, torch.int64, "nbr", contiguous=False), ld_n, k,
          ops._p(rank, torch.int32, "rank_out", contiguous=False), ld_r, penalty,
          ws=ops._ws(load().mmg_nn_rank_ws_bytes(n, D, k), x.device))
    return rank, penalty
