"""The host restatement of the fp64 Cholesky solve (mmgnn/cholesky.py; csrc/chol64.h on the device) -- no GPU needed.
The GPU tests hold the three kernels EQUAL to ``chained.host_solve``, ``lowrank.host_solve`` and
``missingness.host_solve``, so these must not move:

* ``host_cholesky_solve`` is held EQUAL, the count of bad pivots included, to a scalar loop that does one operation
  per element, at m = 1, 2, 3, 17, 33, 129 and on a negative-definite system;
* the three public functions are held to SHA-256 digests of their outputs.  Every literal was recorded from the commit
  BEFORE the three functions moved onto the shared one (each restated the loops then), so a change of the shared
  arithmetic or of how a caller builds its system cannot pass quietly.

Every input comes from a closed formula over small integers: nothing depends on a generator's stream, and B^T B is
exact in fp64 whatever order a BLAS adds it in."""
import hashlib

import numpy as np
import pytest


def ints(rows, cols, salt):
    """Small integers in [-5, 5] from a closed formula."""
    i, k = np.arange(rows)[:, None], np.arange(cols)[None, :]
    return ((i * 7 + k * 13 + i * k * 3 + salt * 5) % 11 - 5).astype(np.float64)


def spd(m, salt):
    """B^T B / 64 + I with B [m + 3, m] small integers: symmetric positive definite, exact up to the + I."""
    B = ints(m + 3, m, salt)
    return B.T @ B / 64.0 + np.eye(m)


def vec(m, salt):
    return ((np.arange(m) * 5 + salt * 3) % 7 - 3) / 8.0


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def scalar_solve(A, y):
    """One system, one operation per element, in the order of the contract."""
    A, y = np.array(A, np.float64), np.array(y, np.float64)
    m = y.size
    d, z = np.zeros(m), np.zeros(m)
    bad = 0
    with np.errstate(all="ignore"):
        for k in range(m):
            if not A[k, k] > 0.0:
                bad += 1
            d[k] = np.sqrt(A[k, k])
            for i in range(k + 1, m):
                A[i, k] = A[i, k] / d[k]
            for i in range(k + 1, m):
                for l in range(k + 1, i + 1):
                    A[i, l] = A[i, l] - A[i, k] * A[l, k]
        for k in range(m):
            z[k] = y[k] / d[k]
            for i in range(k + 1, m):
                y[i] = y[i] - A[i, k] * z[k]
        for k in range(m - 1, -1, -1):
            y[k] = z[k] / d[k]
            for i in range(k):
                z[i] = z[i] - A[k, i] * y[k]
    return y, bad


@pytest.mark.parametrize("m", [1, 2, 3, 17, 33, 129])
def test_host_cholesky_solve_equals_the_scalar_loop(m):
    from mmgnn.cholesky import host_cholesky_solve
    A, y = spd(m, m), vec(m, m)
    x, bad = host_cholesky_solve(A[None], y[None])
    want, want_bad = scalar_solve(A, y)
    assert x.shape == (1, m) and np.isfinite(x).all()
    assert np.array_equal(x[0], want) and bad == want_bad == 0
    # the solution of the system: the rounding statement of the docstring, with |A| |x| taken entrywise
    assert (np.abs(A @ x[0] - y) <= 8 * m * m * 2.0 ** -53 * (np.abs(A) @ np.abs(x[0]))).all()


def test_host_cholesky_solve_counts_pivots_that_are_not_positive():
    from mmgnn.cholesky import host_cholesky_solve
    m = 5
    A = np.stack([spd(m, 1), -spd(m, 2), spd(m, 3)])               # the middle one is negative definite
    A[2, 3, 3] = A[2, 3, 3] - 40.0                                 # ... the last one fails at its fourth pivot
    y = np.stack([vec(m, 1), vec(m, 2), vec(m, 3)])
    x, bad = host_cholesky_solve(A, y)
    want = [scalar_solve(A[s], y[s]) for s in range(3)]
    assert [w[1] for w in want] == [0, m, 2]                       # NaN from the first bad pivot on: each later one counts
    assert bad == 0 + m + 2
    for s in range(3):
        assert np.array_equal(x[s], want[s][0], equal_nan=True)
    assert np.isfinite(x[0]).all() and np.isnan(x[1]).all()


def test_host_cholesky_solve_leaves_its_arguments_alone():
    from mmgnn.cholesky import host_cholesky_solve
    A, y = spd(4, 0)[None], vec(4, 0)[None]
    A0, y0 = A.copy(), y.copy()
    host_cholesky_solve(A, y)
    assert np.array_equal(A, A0) and np.array_equal(y, y0)


# ---- the three public restatements against the digests of their outputs before the move
def chain_case(L, j, inactive):
    G, s = spd(L, L), vec(L, L + 1) * 4.0
    count = np.arange(L, dtype=np.int64) % 4 + 1
    count[inactive] = 0
    return G, s, 37, count, j, 0.5


def prop_case(D):
    M = D + 1
    return spd(M, D), vec(M, D) * 2.0, vec(M, D + 2) + 0.0625, 0.75     # trial != 0; the intercept is not penalised


def mf_case(r):
    return np.stack([spd(r, 10 + s) for s in range(3)]), np.stack([vec(r, 20 + s) for s in range(3)])


CHAIN = {(9, 4, 2): "e00f678eeb29cfdb0f8696c9e5277cae295dcd644e1f7f97506c23cccc5694aa",      # (L, j, the inactive lab)
         (40, 17, 0): "147987aabb10a2ea8db8e3f5264beae30cb58246358852e87c3bd8b3186094d2"}
PROP = {5: "5c077fa5790dd813b5112eee118e55aab2fdca098853a0b6a4d5b8d22ea7bf05",                # D
        32: "ab454fdcafdb8b539bf68b4ed00a18f0dcc06f00cc880c38923faf2746e58d95"}
MF = {5: "27a0a21c1ba4a8153aca17825b999acd02d1e12a847e2c3b260841860ea2853e",                  # rank, S = 3 systems at once
      32: "473a6a51d8be346f4b9632098a29b73bf81c5c4f0cbad5c13f6dd4870fe9e821"}


@pytest.mark.parametrize("case", list(CHAIN))
def test_chained_host_solve_is_the_recorded_one(case):
    from mmgnn import chained
    L, j, inactive = case
    w, mu, bad = chained.host_solve(*chain_case(*case))
    assert w.shape == mu.shape == (L,) and bad == 0
    assert w[j] == 0.0 and w[inactive] == 0.0 and np.count_nonzero(w) == L - 2
    assert digest(w, mu) == CHAIN[case]


@pytest.mark.parametrize("D", list(PROP))
def test_missingness_host_solve_is_the_recorded_one(D):
    from mmgnn import missingness
    H, g, trial, C = prop_case(D)
    assert trial.all()
    delta, dec, bad = missingness.host_solve(H, g, trial, C)
    assert delta.shape == (D + 1,) and bad == 0 and dec > 0.0
    assert digest(delta, np.float64(dec)) == PROP[D]


@pytest.mark.parametrize("r", list(MF))
def test_lowrank_host_solve_is_the_recorded_one(r):
    from mmgnn import lowrank
    x, bad = lowrank.host_solve(*mf_case(r))
    assert x.shape == (3, r) and bad == 0
    assert digest(x) == MF[r]
