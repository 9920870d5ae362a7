"""The one float64 Cholesky solve of the package on the host: the arithmetic of csrc/chol64.h (and of the solve inside
csrc/mf.hip's k_mf_segment), operation by operation.  ``chained.host_solve``, ``lowrank.host_solve`` and
``missingness.host_solve`` build their systems and call it; the GPU tests hold ``mmg_chain_solve``,
``mmg_mf_half_sweep`` and ``mmg_prop_solve`` EQUAL to them.
"""
from __future__ import annotations

import numpy as np


def host_cholesky_solve(A, y):
    """x = A^{-1} y for every system of A [S, m, m] (symmetric; the lower triangle is read), y [S, m] -> (x fp64 [S, m],
    pivots not > 0 over all the systems).  A right-looking in-place factorisation -- d_k = sqrt(A_kk), column k divided
    by d_k, the trailing update A_il - A_ik A_lk -- then the two column-oriented substitutions, each dividing by d_k; a
    product and a sum are two roundings (no fused multiply-add).  A pivot that is not > 0 is counted and the arithmetic
    goes on (NaN or inf from there).  Rounding: a backward-stable Cholesky solve, |A x - b| <= 8 m^2 2^-53 |A| |x| to
    first order."""
    A, y = np.array(A, np.float64), np.array(y, np.float64)
    S, m = y.shape
    d = np.zeros((S, m))
    bad = 0
    with np.errstate(all="ignore"):
        for k in range(m):
            bad += int((~(A[:, k, k] > 0.0)).sum())
            d[:, k] = np.sqrt(A[:, k, k])
            A[:, k + 1:, k] = A[:, k + 1:, k] / d[:, k, None]
            A[:, k + 1:, k + 1:] = A[:, k + 1:, k + 1:] - A[:, k + 1:, k, None] * A[:, None, k + 1:, k]
        for k in range(m):
            y[:, k] = y[:, k] / d[:, k]
            y[:, k + 1:] = y[:, k + 1:] - A[:, k + 1:, k] * y[:, k, None]
        for k in range(m - 1, -1, -1):
            y[:, k] = y[:, k] / d[:, k]
            y[:, :k] = y[:, :k] - A[:, k, :k] * y[:, k, None]
    return y, bad
