"""float64 numpy restatement of mmg_knn_impute / KNNLabImputer: sklearn.impute.KNNImputer(n_neighbors=k, weights=w)
.fit_transform(X) with the all-missing columns kept (as NaN) and ties broken by the lower donor index.  The oracle of
tests/test_knn_*.py.

  dist(r, d) = sqrt(L * S / c), c = labs both rows observe, S = sum over them of (X[r, j] - X[d, j])^2 (direct sum, no
  expansion), NaN when c = 0.  Missing cell (r, l): donors = rows observing l; none -> NaN; all at a NaN distance ->
  fp32(fp64 mean of the observed X[:, l]); else the min(k, |donors|) donors of smallest (dist, d), NaN last, averaged
  with weights 1 (uniform) or 1 / dist ([dist == 0] when a chosen distance is 0), NaN distances weighing 0.

Distances are computed per block of receivers, chunked over the donors, so 256 receivers x 183,400 donors fit in memory.
"""
from __future__ import annotations

import numpy as np


def pair_q(Xr: np.ndarray, Xd: np.ndarray, chunk: int = 4096) -> np.ndarray:
    """S / c in float64 for every (receiver, donor) pair, NaN where c = 0.  Xr [n, L], Xd [N, L], NaN = missing."""
    Xr = np.asarray(Xr, np.float64)
    Xd = np.asarray(Xd, np.float64)
    mr = ~np.isnan(Xr)
    q = np.empty((Xr.shape[0], Xd.shape[0]), np.float64)
    for d0 in range(0, Xd.shape[0], chunk):
        xd = Xd[d0:d0 + chunk]
        md = ~np.isnan(xd)
        S = np.zeros((Xr.shape[0], xd.shape[0]), np.float64)
        c = np.zeros((Xr.shape[0], xd.shape[0]), np.int64)
        for j in range(Xr.shape[1]):
            rj = np.flatnonzero(mr[:, j])
            dj = np.flatnonzero(md[:, j])
            if rj.size == 0 or dj.size == 0:
                continue
            diff = Xr[rj, j][:, None] - xd[dj, j][None, :]
            S[np.ix_(rj, dj)] += diff * diff
            c[np.ix_(rj, dj)] += 1
        with np.errstate(invalid="ignore", divide="ignore"):
            q[:, d0:d0 + chunk] = np.where(c > 0, S / np.maximum(c, 1), np.nan)
    return q


def knn_impute_ref(X: np.ndarray, rows=None, k: int = 5, weights: str = "uniform", block: int = 64,
                   return_gap: bool = False):
    """-> out [len(rows), L] float64 (and, with return_gap, the relative gap between the k'-th and (k'+1)-th distance of
    every missing cell: 0 = an exact tie at the selection boundary, inf = no (k'+1)-th finite distance or no selection)."""
    X = np.asarray(X, np.float64)
    N, L = X.shape
    rows = np.arange(N) if rows is None else np.asarray(rows, np.int64)
    obs = ~np.isnan(X)
    cnt = obs.sum(0)
    with np.errstate(invalid="ignore"):
        col_mean = np.where(cnt > 0, np.float32(np.nansum(X, 0) / np.maximum(cnt, 1)), np.nan).astype(np.float64)
    out = X[rows].copy()
    gap = np.full(out.shape, np.inf)
    for b0 in range(0, len(rows), block):
        rb = rows[b0:b0 + block]
        dist = np.sqrt(L * pair_q(X[rb], X))               # [B, N], NaN where no common lab
        for bi, r in enumerate(rb):
            i = b0 + bi
            for l in np.flatnonzero(~obs[r]):
                if cnt[l] == 0:
                    out[i, l] = np.nan
                    continue
                dl = dist[bi, obs[:, l]]                    # donors of lab l, in row order (r is never one)
                xl = X[obs[:, l], l]
                fin = np.flatnonzero(~np.isnan(dl))
                if fin.size == 0:
                    out[i, l] = col_mean[l]
                    continue
                kk = min(k, fin.size)
                if fin.size > kk + 1:                       # only the donors up to the (kk+1)-th distance need sorting
                    df = dl[fin]
                    fin = fin[df <= df[np.argpartition(df, kk)[kk]]]
                order = fin[np.lexsort((fin, dl[fin]))]    # (dist, row) ascending
                sel = order[:kk]
                ds, xs = dl[sel], xl[sel]
                if weights == "uniform":
                    w = np.ones(kk)
                elif np.any(ds == 0):
                    w = (ds == 0).astype(np.float64)
                else:
                    w = 1.0 / ds
                out[i, l] = np.sum(w * xs) / np.sum(w)
                if fin.size > kk:
                    a, b = dl[order[kk - 1]], dl[order[kk]]
                    gap[i, l] = (b - a) / max(abs(b), 1e-30)
    return (out, gap) if return_gap else out
