"""Loop reference of lab imputation by chained equations (mmgnn/chained.py, csrc/chain.hip): the moments of one step by
math.fsum (the correctly rounded sum of its float64 terms), and the whole chain -- means, centred normal equations,
Cholesky, prediction -- in 80-bit numpy.longdouble, written from the textbook form (centre the predictors and the
target over the rows that have the target, solve (Z^T Z + alpha I) w = Z^T y) instead of the moment form of the
definition.  Independent of the numpy restatement.  Also the test matrices."""
import math

import numpy as np

import assoc_ref

F32 = np.float32
LD = np.longdouble
U = 2.0 ** -53


def make_matrix(n, L, seed=0, density=0.6, lattice=False):
    """fp32 [n, L] with NaN for missing, every lab with at least two values (assoc_ref.make_matrix without its special
    cells)."""
    X = assoc_ref.make_matrix(n, L, seed, density, lattice=lattice, special=False)
    for a in range(L):
        if np.isfinite(X[:, a]).sum() < min(2, n):
            X[:min(2, n), a] = np.array([0.5, 1.5], F32)[:min(2, n)] + F32(a % 3)
    return X


def moments(W, X, j, center):
    """-> (n_j, s [L], G [L, L] by fsum, the absolute sums of the same terms: sa [L], Ga [L, L]).  The terms are the
    float64 values the definition names: u = W - center (one rounding), u_a * u_b (one rounding)."""
    rows = np.flatnonzero(np.isfinite(np.asarray(X, F32)[:, j]))
    L = W.shape[1]
    c = np.asarray(center, np.float64)
    u = [W[rows, a] - c[a] for a in range(L)]
    s, sa = np.zeros(L), np.zeros(L)
    G, Ga = np.zeros((L, L)), np.zeros((L, L))
    for a in range(L):
        s[a] = math.fsum(u[a].tolist())
        sa[a] = math.fsum(np.abs(u[a]).tolist())
        for b in range(a, L):
            prod = u[a] * u[b]
            G[a, b] = G[b, a] = math.fsum(prod.tolist())
            Ga[a, b] = Ga[b, a] = math.fsum(np.abs(prod).tolist())
    return rows.size, s, G, sa, Ga


def moment_bound(n_j, ab):
    """|moment - fsum| allowed: (n_j + 8) 2^-53 x the sum of the absolute terms (the form and the reasoning of
    assoc_ref.moment_bound: any order of n_j terms, a product formed inside a fused multiply-add, second order)."""
    return (n_j + 8.0) * U * ab


def visit_order(X, name):
    """The labs somebody has, in the order of a round."""
    X = np.asarray(X, F32)
    n, L = X.shape
    missing = [int(np.isnan(X[:, a]).sum()) for a in range(L)]
    labs = list(range(L))
    if name == "ascending":
        labs = sorted(labs, key=lambda a: missing[a])                  # stable: ties left to right
    elif name == "descending":
        labs = sorted(labs, key=lambda a: missing[a])[::-1]
    elif name == "arabic":
        labs = labs[::-1]
    else:
        assert name == "roman"
    return [a for a in labs if missing[a] < n]


def _cholesky_solve(A, b):
    """A w = b for a symmetric positive definite A, 80-bit, row by row (Cholesky-Banachiewicz)."""
    m = b.size
    Lo = np.zeros((m, m), LD)
    for i in range(m):
        for k in range(i):
            Lo[i, k] = (A[i, k] - np.dot(Lo[i, :k], Lo[k, :k])) / Lo[k, k]
        Lo[i, i] = np.sqrt(A[i, i] - np.dot(Lo[i, :i], Lo[i, :i]))
    y = np.zeros(m, LD)
    for i in range(m):
        y[i] = (b[i] - np.dot(Lo[i, :i], y[:i])) / Lo[i, i]
    w = np.zeros(m, LD)
    for i in range(m - 1, -1, -1):
        w[i] = (y[i] - np.dot(Lo[i + 1:, i], w[i + 1:])) / Lo[i, i]
    return w


def chain(X, alpha=1.0, rounds=10, order="ascending", lo=None, hi=None, tol=0.0):
    """-> (W longdouble [n, L] -- NaN in the columns nobody has --, the visit order, the delta of every round)."""
    assert np.finfo(LD).nmant >= 63, "no 80-bit long double on this platform"
    X = np.asarray(X, F32)
    n, L = X.shape
    obs = np.isfinite(X)
    labs = visit_order(X, order)
    active = np.array(sorted(labs), int)
    W = np.where(obs, X.astype(LD), LD(0))
    for a in active:
        W[~obs[:, a], a] = W[obs[:, a], a].sum() / LD(int(obs[:, a].sum()))
    lo = np.full(L, -np.inf) if lo is None else np.broadcast_to(np.asarray(lo, np.float64), (L,))
    hi = np.full(L, np.inf) if hi is None else np.broadcast_to(np.asarray(hi, np.float64), (L,))
    threshold = tol * (float(np.abs(X[obs]).max()) if obs.any() else 0.0)
    history = []
    for _ in range(rounds):
        delta = LD(0)
        for j in labs:
            S = obs[:, j]
            P = active[active != j]
            Z, yv = W[S][:, P], W[S, j]
            zm, ym = Z.mean(0) if P.size else np.zeros(0, LD), yv.mean()
            Zc = Z - zm
            w = _cholesky_solve(Zc.T @ Zc + LD(alpha) * np.eye(P.size, dtype=LD), Zc.T @ (yv - ym)) if P.size else Z[0, :0]
            if (~S).any():
                new = ym + (W[~S][:, P] - zm) @ w
                new = np.minimum(np.maximum(new, LD(lo[j])), LD(hi[j]))
                delta = max(delta, np.abs(new - W[~S, j]).max())
                W[~S, j] = new
        history.append(float(delta))
        if float(delta) < threshold:
            break
    W[:, [a for a in range(L) if a not in set(labs)]] = np.nan
    return W, labs, history
