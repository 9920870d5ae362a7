"""ctypes binding and typed entry points of libmmgnn_chain.so (C ABI: include/mmgnn_chain.h; csrc/chain.hip): the
working matrix, the row-masked moments, the ridge solve, the apply and the fp32 result of lab imputation by chained
equations, a library of its own beside libmmgnn.so.  The binding is a ``_lib.Binding`` derived from the header, and
every call goes through ``ops._call``.  The library is REQUIRED: there is no CPU or eager-PyTorch fallback behind these
calls (the numpy restatement of mmgnn/chained.py serves numpy inputs and checks the kernels; it is never a silent
substitute for them).
"""
from __future__ import annotations

import torch

from . import ops

BINDING = ops.satellite("chain", globals())    # LIB_PATH, HEADER_PATH, DEFINES, SIGNATURES, PARAMS, MMG_*, load, _call

CH_MAX_LABS = DEFINES["MMG_CH_MAX_LABS"]
CH_TILE = DEFINES["MMG_CH_TILE"]
CH_CHUNK = DEFINES["MMG_CH_CHUNK"]
CH_APPLY_ROWS = DEFINES["MMG_CH_APPLY_ROWS"]


def chain_plan(n: int, n_labs: int):
    """The slab plan of chain_moments (mmg_chain_plan, a host function) -> (rows per slab, slabs)."""
    return ops.slab_plan(BINDING, "mmg_chain_plan", n, n_labs)


def _working(W: torch.Tensor, n: int, L: int, what: str):
    if not torch.is_tensor(W) or tuple(W.shape) != (n, L) or not W.is_contiguous():
        raise ValueError(f"{what}: W must be a contiguous [{n}, {L}] tensor")


def _vector(v: torch.Tensor, L: int, name: str, what: str):
    if not torch.is_tensor(v) or v.dim() != 1 or v.numel() != L or not v.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous vector of {L} values")


def chain_init(X: torch.Tensor, center: torch.Tensor) -> torch.Tensor:
    """W fp64 [n, L]: X where observed, else center (mmg_chain_init)."""
    px, n, L, ld = ops._lab_matrix(X, "chain_init")
    _vector(center, L, "center", "chain_init")
    W = torch.empty(n, L, dtype=torch.float64, device=X.device)
    _call("mmg_chain_init", px, n, L, ld, center, W)
    return W


def chain_moments(W: torch.Tensor, X: torch.Tensor, j: int, center: torch.Tensor, out=None):
    """-> (n_j int64 [1], s fp64 [L], G fp64 [L, L]) of u = W - center over the rows that have lab j
    (mmg_chain_moments).  out: the three tensors of an earlier call, written again."""
    px, n, L, ld = ops._lab_matrix(X, "chain_moments")
    _working(W, n, L, "chain_moments")
    _vector(center, L, "center", "chain_moments")
    if out is None:
        out = (torch.empty(1, dtype=torch.int64, device=X.device), torch.empty(L, dtype=torch.float64, device=X.device),
               torch.empty(L, L, dtype=torch.float64, device=X.device))
    n_j, s, G = out
    _call("mmg_chain_moments", W, px, n, L, ld, int(j), center, n_j, s, G,
          ws=ops._ws(load().mmg_chain_moments_ws_bytes(n, L), X.device))
    return out


def chain_solve(G: torch.Tensor, s: torch.Tensor, n_j: torch.Tensor, count: torch.Tensor, j: int, alpha: float,
                w: torch.Tensor, mu: torch.Tensor, bad: torch.Tensor):
    """The ridge coefficients of target j into w, mu (fp64 [L] each); bad (int64 [1]) += the pivots that were not
    positive (mmg_chain_solve)."""
    L = int(s.numel())
    if G.dim() != 2 or tuple(G.shape) != (L, L) or not G.is_contiguous():
        raise ValueError(f"chain_solve: G must be a contiguous [{L}, {L}] tensor, got {tuple(G.shape)}")
    for v, name in ((s, "s"), (count, "count"), (w, "w"), (mu, "mu")):
        _vector(v, L, name, "chain_solve")
    _call("mmg_chain_solve", G, s, n_j, count, L, int(j), float(alpha), w, mu, bad)


def chain_apply(W: torch.Tensor, X: torch.Tensor, j: int, count: torch.Tensor, center: torch.Tensor, w: torch.Tensor,
                mu: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, delta: torch.Tensor, accumulate: bool = False):
    """Rewrite column j of W on the rows without lab j; delta (fp64 [1]) = the largest |new - old|, folded into its
    value when ``accumulate`` (mmg_chain_apply)."""
    px, n, L, ld = ops._lab_matrix(X, "chain_apply")
    _working(W, n, L, "chain_apply")
    for v, name in ((count, "count"), (center, "center"), (w, "w"), (mu, "mu"), (lo, "lo"), (hi, "hi")):
        _vector(v, L, name, "chain_apply")
    _call("mmg_chain_apply", W, px, n, L, ld, int(j), count, center, w, mu, lo, hi, int(bool(accumulate)), delta,
          ws=ops._ws(load().mmg_chain_apply_ws_bytes(n, L), X.device))


def chain_finish(W: torch.Tensor, X: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    """fp32 [n, L]: observed cells bit for bit, NaN for a lab nobody has, else W rounded once (mmg_chain_finish)."""
    px, n, L, ld = ops._lab_matrix(X, "chain_finish")
    _working(W, n, L, "chain_finish")
    _vector(count, L, "count", "chain_finish")
    out = torch.empty(n, L, dtype=torch.float32, device=X.device)
    _call("mmg_chain_finish", W, px, n, L, ld, count, out, L)
    return out
