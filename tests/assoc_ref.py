"""Loop reference of the lab association tables (mmgnn/association.py, csrc/assoc.hip): per lab pair the co-observed
rows, every sum by math.fsum (the correctly rounded sum of its float64 terms), the finish in 80-bit numpy.longdouble.
Independent of the numpy restatement: no matrix product, no mask arithmetic.  Also the test matrices."""
import math

import numpy as np

F32 = np.float32
LD = np.longdouble
U = 2.0 ** -53


def observed(X):
    return np.isfinite(np.asarray(X, F32))


def colstats(X):
    """-> (count int64 [L], fsum of the observed values [L], sum of their absolute values [L], infinite cells)."""
    X = np.asarray(X, F32)
    obs = observed(X)
    L = X.shape[1]
    count = np.zeros(L, np.int64)
    s, sa = np.zeros(L), np.zeros(L)
    for a in range(L):
        v = [float(x) for x in X[obs[:, a], a]]
        count[a] = len(v)
        s[a] = math.fsum(v)
        sa[a] = math.fsum(abs(x) for x in v)
    return count, s, sa, int(np.isinf(X).sum())


def moments(X, center):
    """-> (planes fp64 [4, L, L]: N, SX, SXX, SXY by fsum; absolute sums [4, L, L] of the same terms).  The terms are
    the float64 values the definition names: u = float64(x) - center (one rounding), q = u * u and u_a * u_b (one
    rounding each)."""
    X = np.asarray(X, F32)
    obs = observed(X)
    n, L = X.shape
    c = np.asarray(center, np.float64)
    u = [np.where(obs[:, a], X[:, a].astype(np.float64) - c[a], 0.0) for a in range(L)]     # one rounding per cell
    out, ab = np.zeros((4, L, L)), np.zeros((4, L, L))
    for a in range(L):
        for b in range(a, L):
            both = np.flatnonzero(obs[:, a] & obs[:, b])                 # the co-observed rows of the pair
            ua, ub = u[a][both], u[b][both]
            out[0, a, b] = out[0, b, a] = ab[0, a, b] = ab[0, b, a] = both.size
            for x, p, q in ((ua, a, b), (ub, b, a)):                     # SX[a, b] sums u_a, SX[b, a] sums u_b
                out[1, p, q] = math.fsum(x.tolist())
                ab[1, p, q] = math.fsum(np.abs(x).tolist())
                out[2, p, q] = ab[2, p, q] = math.fsum((x * x).tolist())
            prod = ua * ub                                               # elementwise: each product rounded once
            out[3, a, b] = out[3, b, a] = math.fsum(prod.tolist())
            ab[3, a, b] = ab[3, b, a] = math.fsum(np.abs(prod).tolist())
    return out, ab


def moment_bound(ab):
    """|moment - fsum| allowed: (nab + 8) 2^-53 x the sum of the absolute terms.  A sum of nab float64 terms in ANY order
    is within (nab - 1) u of the exact sum relative to the absolute sum (first order), fsum within u / 2 of it, a product
    formed inside a fused multiply-add instead of rounded on its own moves its term by u: nab + 1/2 in all, and the 8 covers
    the second-order part."""
    return (ab[0] + 8.0) * U * ab


def finish(planes, count, n, min_periods=1):
    """(r, cov, jaccard, lift) as float64 from an 80-bit evaluation of the definition; the same NaN rules."""
    assert np.finfo(LD).nmant >= 63, "no 80-bit long double on this platform"
    L = planes.shape[1]
    r, cov, jac, lift = (np.full((L, L), np.nan) for _ in range(4))
    for a in range(L):
        for b in range(L):
            nab = int(planes[0, a, b])
            ca, cb = int(count[a]), int(count[b])
            if ca + cb - nab:
                jac[a, b] = nab / (ca + cb - nab)
            if ca * cb:
                lift[a, b] = (nab * int(n)) / (ca * cb)
            if nab < 1:
                continue
            sx, sy, sxx, syy, sxy = (LD(v) for v in (planes[1, a, b], planes[1, b, a], planes[2, a, b], planes[2, b, a],
                                                     planes[3, a, b]))
            cxy, vx, vy = sxy - sx * sy / LD(nab), sxx - sx * sx / LD(nab), syy - sy * sy / LD(nab)
            if nab >= max(min_periods, 2):
                cov[a, b] = float(cxy / LD(nab - 1))
            # one common row has no variance: vx = q - u * u is 0 by definition, which the 80-bit product of the
            # float64-rounded q does not reproduce
            if nab >= max(min_periods, 2) and vx * vy > 0:
                r[a, b] = float(min(max(cxy / np.sqrt(vx * vy), LD(-1)), LD(1)))
    return r, cov, jac, lift


# ---------------------------------------------------------------------------------- matrices
def make_matrix(n, L, seed=0, density=0.6, lattice=False, special=True):
    """fp32 [n, L] with NaN for missing.  Generic: correlated columns (a shared patient factor), per-lab offset and scale.
    lattice: small multiples of 1/8, so that every sum about a lattice centre is exact.  special (L >= 6, n >= 8): lab 1
    all-missing, lab 2 constant, row 3 all-NaN, labs 3 / 4 / 5 share 0, 1 and 2 rows pairwise in places."""
    rng = np.random.default_rng(seed)
    if lattice:
        X = (rng.integers(-40, 41, (n, L)) / 8.0).astype(F32)
    else:
        f = rng.standard_normal((n, 1))
        load = rng.uniform(-1.0, 1.0, (1, L))
        X = (f * load + rng.standard_normal((n, L))) * rng.uniform(0.5, 3.0, (1, L)) + rng.uniform(-5.0, 5.0, (1, L))
        X = X.astype(F32)
    X[rng.random((n, L)) >= density] = np.nan
    if special and L >= 6 and n >= 8:
        X[:, 1] = np.nan
        X[~np.isnan(X[:, 2]), 2] = F32(2.5)
        X[3, :] = np.nan
        X[:, 3:6] = np.nan
        X[0, 3], X[1, 3], X[2, 3] = F32(1.0), F32(2.0), F32(-1.0)   # lab 3: rows 0, 1, 2
        X[2, 4] = X[4, 4] = X[5, 4] = F32(-0.5)          # lab 4: rows 2, 4, 5    -> (3, 4) share 1 row
        X[4, 4] = F32(0.25)
        X[0, 5], X[1, 5], X[6, 5], X[7, 5] = F32(0.5), F32(1.5), F32(-1.0), F32(2.0)   # (3, 5) share 2, (4, 5) share 0
    return X


def lattice_center(L, seed=0):
    return np.random.default_rng(seed + 1000).integers(-16, 17, L) / 8.0


# (n, L, density, min_periods, seed): every one with make_matrix's special cells -- an all-missing lab, a constant
# lab, an all-NaN patient, pairs with 0, 1 and 2 common rows -- and a lab with mean 1e4 and std 1 (lab 0).  min_periods
# blanks some cells of a shape and never all off-diagonal ones: on the diagonal alone pandas is exactly 1 and its
# distance from the reference, the yardstick, would be 0.
PANDAS_SHAPES = [(8, 6, 0.9, 1, 0), (40, 6, 0.5, 1, 1), (40, 7, 0.5, 3, 2), (97, 9, 0.3, 1, 3), (97, 9, 0.3, 8, 4),
                 (300, 17, 0.6, 1, 5), (300, 17, 0.15, 5, 6), (1000, 8, 0.7, 30, 7), (33, 20, 0.4, 2, 8), (513, 12, 0.05, 1, 9)]


def pandas_case(n, L, density, seed):
    X = make_matrix(n, L, seed, density)
    col = X[:, 0]
    col[~np.isnan(col)] += F32(1e4)                       # mean 1e4, std of order 1: why the moments are centred
    return X
