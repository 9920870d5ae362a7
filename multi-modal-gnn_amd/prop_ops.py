"""ctypes binding and typed entry points of libmmgnn_prop.so (C ABI: include/mmgnn_prop.h; csrc/prop.hip): the
indicator, the link, the weighted moments, the Newton solve, the per-lab state machine and the propensities of the
per-lab measurement models and the weighted error sums over pairs, a library of its own beside libmmgnn.so.  The binding is a ``_lib.Binding`` derived from the
header, and every call goes through ``ops._call``.  The library is REQUIRED: there is no CPU or eager-PyTorch fallback
behind these calls (the numpy restatement of mmgnn/missingness.py serves numpy inputs and checks the kernels; it is never
a silent substitute for them).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops

BINDING = ops.satellite("prop", globals())     # LIB_PATH, HEADER_PATH, DEFINES, SIGNATURES, PARAMS, MMG_*, load, _call

PR_MAX_FEATURES = DEFINES["MMG_PR_MAX_FEATURES"]
PR_MAX_LABS = DEFINES["MMG_PR_MAX_LABS"]
PR_MAX_BATCH = DEFINES["MMG_PR_MAX_BATCH"]
PR_CHUNK = DEFINES["MMG_PR_CHUNK"]
PR_LINK_ROWS = DEFINES["MMG_PR_LINK_ROWS"]
PR_STATE = DEFINES["MMG_PR_STATE"]
PR_FSTATE = DEFINES["MMG_PR_FSTATE"]
PR_PAIR_CHUNK = DEFINES["MMG_PR_PAIR_CHUNK"]
PR_PAIR_FIELDS = DEFINES["MMG_PR_PAIR_FIELDS"]
ACTIVE, N_ITER, CONVERGED, HALVINGS, STARTED, BAD = (DEFINES["MMG_PR_" + k] for k in
                                                     ("ACTIVE", "N_ITER", "CONVERGED", "HALVINGS", "STARTED", "BAD"))


def prop_plan(n: int, n_features: int):
    """The slab plan of prop_moments (mmg_prop_plan, a host function) -> (rows per slab, slabs)."""
    return ops.slab_plan(BINDING, "mmg_prop_plan", n, n_features)


def prop_batch(n: int, n_features: int) -> int:
    """The labs one call works on (mmg_prop_batch, a host function); 0: unsupported shape."""
    return int(load().mmg_prop_batch(int(n), int(n_features)))


def link_blocks(n: int) -> int:
    return (int(n) + PR_LINK_ROWS - 1) // PR_LINK_ROWS


def _labels(Y: torch.Tensor, n: int, what: str):
    if not torch.is_tensor(Y) or Y.dim() != 2 or Y.shape[0] != n or (Y.shape[1] > 1 and Y.stride(1) != 1):
        raise ValueError(f"{what}: Y must be a [{n}, labs] tensor with unit column stride")
    L = int(Y.shape[1])
    return ops._p(Y, (torch.uint8, torch.bool), "Y", contiguous=False), L, int(Y.stride(0)) if n > 1 else max(int(Y.stride(0)), L)


def _shaped(t: torch.Tensor, shape, name: str, what: str):
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous {list(shape)} tensor")
    return t


def prop_indicator(X: torch.Tensor, features: bool = False):
    """-> Y uint8 [n, L] = isfinite(X) (and the same as fp32 0 / 1 when ``features``) (mmg_prop_indicator)."""
    px, n, L, ld = ops._lab_matrix(X, "prop_indicator")
    Y = torch.empty(n, L, dtype=torch.uint8, device=X.device)
    F = torch.empty(n, L, dtype=torch.float32, device=X.device) if features else None
    _call("mmg_prop_indicator", px, n, L, ld, Y, L, F, L)
    return (Y, F) if features else Y


def prop_count(Y: torch.Tensor) -> torch.Tensor:
    """-> int64 [L]: the rows that have each lab (mmg_prop_count)."""
    n = int(Y.shape[0]) if torch.is_tensor(Y) and Y.dim() == 2 else 0
    py, L, ld_y = _labels(Y, n, "prop_count")
    count = torch.empty(L, dtype=torch.int64, device=Y.device)
    _call("mmg_prop_count", py, n, L, ld_y, count)
    return count


def prop_link(X: torch.Tensor, mean: torch.Tensor, Y: torch.Tensor, j0: int, nb: int, coef: torch.Tensor,
              state: Optional[torch.Tensor], sr: torch.Tensor, lossp: torch.Tensor, z: Optional[torch.Tensor] = None,
              pq: Optional[torch.Tensor] = None):
    """s, r (sr fp64 [2, nb, n]) and the loss block sums (lossp fp64 [nb, blocks]) of the labs j0 .. j0 + nb - 1 at the
    coefficients coef (fp64 [L, D + 1]); z (fp64 [nb, n]) and pq (fp64 [2, nb, n]) where given (mmg_prop_link)."""
    px, n, D, ld = ops._lab_matrix(X, "prop_link")
    py, L, ld_y = _labels(Y, n, "prop_link")
    _shaped(mean, (D,), "mean", "prop_link")
    _shaped(coef, (L, D + 1), "coef", "prop_link")
    _shaped(sr, (2, nb, n), "sr", "prop_link")
    _shaped(lossp, (nb, link_blocks(n)), "lossp", "prop_link")
    if state is not None:
        _shaped(state, (L, PR_STATE), "state", "prop_link")
    if z is not None:
        _shaped(z, (nb, n), "z", "prop_link")
    if pq is not None:
        _shaped(pq, (2, nb, n), "pq", "prop_link")
    _call("mmg_prop_link", px, n, D, ld, mean, py, ld_y, L, int(j0), int(nb), coef, state, z, pq, sr, lossp)


def prop_moments(X: torch.Tensor, mean: torch.Tensor, sr: torch.Tensor, L: int, j0: int, nb: int,
                 state: Optional[torch.Tensor], H: torch.Tensor, g: torch.Tensor):
    """H (fp64 [nb, D + 1, D + 1]) and g (fp64 [nb, D + 1]) of the batch from s, r (mmg_prop_moments)."""
    px, n, D, ld = ops._lab_matrix(X, "prop_moments")
    _shaped(mean, (D,), "mean", "prop_moments")
    _shaped(sr, (2, nb, n), "sr", "prop_moments")
    _shaped(H, (nb, D + 1, D + 1), "H", "prop_moments")
    _shaped(g, (nb, D + 1), "g", "prop_moments")
    if state is not None:
        _shaped(state, (L, PR_STATE), "state", "prop_moments")
    _call("mmg_prop_moments", px, n, D, ld, mean, sr, int(L), int(j0), int(nb), state, H, g,
          ws=ops._ws(load().mmg_prop_moments_ws_bytes(n, D, int(nb)), X.device))


def prop_solve(H: torch.Tensor, g: torch.Tensor, trial: torch.Tensor, j0: int, C: float, state: torch.Tensor,
               delta: torch.Tensor, dec: torch.Tensor):
    """The Newton direction (delta fp64 [nb, D + 1]) and decrement (dec fp64 [nb]) of the batch at trial (fp64
    [L, D + 1]); state[:, BAD] += the pivots that were not positive (mmg_prop_solve)."""
    if not torch.is_tensor(g) or g.dim() != 2:
        raise ValueError("prop_solve: g must be [nb, D + 1]")
    nb, M = (int(v) for v in g.shape)
    L = int(trial.shape[0]) if torch.is_tensor(trial) and trial.dim() == 2 else 0
    _shaped(g, (nb, M), "g", "prop_solve")
    _shaped(H, (nb, M, M), "H", "prop_solve")
    _shaped(trial, (L, M), "trial", "prop_solve")
    _shaped(state, (L, PR_STATE), "state", "prop_solve")
    _shaped(delta, (nb, M), "delta", "prop_solve")
    _shaped(dec, (nb,), "dec", "prop_solve")
    _call("mmg_prop_solve", H, g, trial, M - 1, L, int(j0), nb, float(C), state, delta, dec)


def prop_update(lossp: torch.Tensor, n: int, j0: int, delta: torch.Tensor, dec: torch.Tensor, C: float, threshold: float,
                max_iter: int, beta: torch.Tensor, trial: torch.Tensor, step: torch.Tensor, fstate: torch.Tensor,
                state: torch.Tensor):
    """One round of the per-lab state machine for the batch (mmg_prop_update)."""
    if not torch.is_tensor(delta) or delta.dim() != 2 or not torch.is_tensor(beta) or beta.dim() != 2:
        raise ValueError("prop_update: delta must be [nb, D + 1] and beta [L, D + 1]")
    nb, M = (int(v) for v in delta.shape)
    L = int(beta.shape[0])
    _shaped(delta, (nb, M), "delta", "prop_update")
    _shaped(lossp, (nb, link_blocks(n)), "lossp", "prop_update")
    _shaped(dec, (nb,), "dec", "prop_update")
    for t, name in ((beta, "beta"), (trial, "trial"), (step, "step")):
        _shaped(t, (L, M), name, "prop_update")
    _shaped(fstate, (L, PR_FSTATE), "fstate", "prop_update")
    _shaped(state, (L, PR_STATE), "state", "prop_update")
    _call("mmg_prop_update", lossp, int(n), M - 1, L, int(j0), nb, delta, dec, float(C), float(threshold), int(max_iter),
          beta, trial, step, fstate, state)


def prop_predict(X: torch.Tensor, mean: torch.Tensor, coef: torch.Tensor, out: Optional[torch.Tensor] = None):
    """-> fp32 [n, L]: the propensity of every lab for every row of X (mmg_prop_predict)."""
    px, n, D, ld = ops._lab_matrix(X, "prop_predict")
    _shaped(mean, (D,), "mean", "prop_predict")
    if not torch.is_tensor(coef) or coef.dim() != 2:
        raise ValueError("prop_predict: coef must be [L, D + 1]")
    L = int(coef.shape[0])
    _shaped(coef, (L, D + 1), "coef", "prop_predict")
    if out is None:
        out = torch.empty(n, L, dtype=torch.float32, device=X.device)
    po, n2, L2, ld_out = ops._rows_matrix(out, "out")
    if (n2, L2) != (n, L):
        raise ValueError(f"prop_predict: out must be [{n}, {L}], got {[n2, L2]}")
    _call("mmg_prop_predict", px, n, D, ld, mean, coef, L, po, ld_out)
    return out


def prop_pair_sums(pred: torch.Tensor, target: torch.Tensor, patient: torch.Tensor, lab: torch.Tensor, P: torch.Tensor,
                   cov: Optional[torch.Tensor], clip: float, stabilized: bool):
    """-> (count int64 [L + 1], sums fp64 [L + 1, 6]): the weighted error sums of the pairs per lab and, in the last row,
    overall (mmg_prop_pair_sums).  pred, target fp32 [m]; patient, lab int64 [m]; P fp32 [n, L]; cov fp64 [L]."""
    pp, n, L, ld_p = ops._rows_matrix(P, "P")
    m = int(pred.numel())
    for t, name in ((pred, "pred"), (target, "target"), (patient, "patient"), (lab, "lab")):
        if not torch.is_tensor(t) or t.dim() != 1 or t.numel() != m or not t.is_contiguous():
            raise ValueError(f"prop_pair_sums: {name} must be a contiguous vector of {m} values")
    if cov is not None:
        _shaped(cov, (L,), "cov", "prop_pair_sums")
    count = torch.empty(L + 1, dtype=torch.int64, device=P.device)
    sums = torch.empty(L + 1, PR_PAIR_FIELDS, dtype=torch.float64, device=P.device)
    _call("mmg_prop_pair_sums", pred, target, patient, lab, m, pp, n, L, ld_p, cov, float(clip), int(bool(stabilized)), count,
          sums, ws=ops._ws(load().mmg_prop_pair_sums_ws_bytes(m, L), P.device))
    return count, sums
