"""Loop reference of the per-lab measurement propensity models (mmgnn/missingness.py, csrc/prop.hip): the link in 80-bit
numpy.longdouble, the weighted moments exactly (integers, on lattice inputs) and in 80-bit sums with the absolute sums
of the same terms (generic inputs), and the whole logistic regression by a textbook Newton iteration in 80-bit
arithmetic, run until its step vanishes.  Independent of the numpy restatement: it never calls the package.  Also the
test data."""
import numpy as np

F32 = np.float32
LD = np.longdouble
U = 2.0 ** -53


# ---------------------------------------------------------------------------------- data
def make_data(kind, n, D, seed):
    """-> (X fp32 [n, D], y uint8 [n]): "generic" (about half positive), "rare" (2-3 % positive), "separable"
    (y = [z > 0])."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)).astype(F32)
    w = rng.standard_normal(D) / np.sqrt(D)
    z = X.astype(np.float64) @ w
    if kind == "generic":
        y = rng.random(n) < 1.0 / (1.0 + np.exp(-z))
    elif kind == "rare":
        y = rng.random(n) < 1.0 / (1.0 + np.exp(-(z - 4.0)))
        y[:max(2, n // 50)] |= z[:max(2, n // 50)] > 0          # never empty
    elif kind == "separable":
        y = z > 0
    else:
        raise ValueError(kind)
    return X, y.astype(np.uint8)


def lattice_case(n, D, seed):
    """Dyadic inputs whose moments are exact in fp64: X multiples of 1/4 in [-4, 4], mean multiples of 1/8, s multiples
    of 1/16 in [0, 1/4], r multiples of 1/16 in [-1, 1]."""
    rng = np.random.default_rng(seed)
    X = (rng.integers(-16, 17, (n, D)) / 4.0).astype(F32)
    mean = rng.integers(-8, 9, D) / 8.0
    s = rng.integers(0, 5, n) / 16.0
    r = rng.integers(-16, 17, n) / 16.0
    return X, mean, s, r


# ---------------------------------------------------------------------------------- link
def link_z(X, mean, coef):
    """-> (80-bit z of one lab at coef = [w, b] over the centred features, sum of |terms|)."""
    u = np.asarray(X, F32).astype(np.float64) - np.asarray(mean, np.float64)[None, :]          # one rounding, as defined
    c = np.asarray(coef, np.float64).astype(LD)
    return u.astype(LD) @ c[:-1] + c[-1], (np.abs(u).astype(LD) @ np.abs(c[:-1]) + np.abs(c[-1])).astype(np.float64)


def link_from_z(z, y):
    """80-bit p, q, s, r and loss terms at the float64 z that the definition pins down."""
    z = np.asarray(z, np.float64).astype(LD)
    e = np.exp(-np.abs(z))
    p = np.where(z >= 0, 1 / (1 + e), e / (1 + e))
    q = np.where(z >= 0, e / (1 + e), 1 / (1 + e))
    yb = np.asarray(y) != 0
    r = np.where(yb, -q, p)
    t = np.maximum(z, 0) - np.where(yb, z, 0) + np.log1p(e)
    return p, q, p * q, r, t


def rel_distance(got, want):
    """The largest |got - want| / |want| of float64 values against 80-bit ones (0 where both are 0)."""
    got, want = np.asarray(got, np.float64).astype(LD), np.asarray(want, LD)
    den = np.where(want == 0, LD(1), np.abs(want))
    return float((np.abs(got - want) / den).max())


# ---------------------------------------------------------------------------------- moments
def _tilde(X, mean, dtype):
    u = np.asarray(X, F32).astype(np.float64) - np.asarray(mean, np.float64)[None, :]          # one rounding, as defined
    return np.concatenate([u, np.ones((u.shape[0], 1))], axis=1).astype(dtype)


def exact_moments(X, mean, s, r):
    """Lattice inputs -> (H [M, M], g [M]) exactly, through integers."""
    ui = np.rint(_tilde(X, mean, np.float64) * 8.0).astype(np.int64)
    si, ri = np.rint(np.asarray(s) * 16.0).astype(np.int64), np.rint(np.asarray(r) * 16.0).astype(np.int64)
    assert np.array_equal(ui / 8.0, _tilde(X, mean, np.float64)) and np.array_equal(si / 16.0, s) and np.array_equal(ri / 16.0, r)
    H = (si[:, None] * ui).T @ ui
    g = ui.T @ ri
    assert int(np.abs(H).max()) < 2 ** 52 and int(np.abs(g).max()) < 2 ** 52
    return H / 1024.0, g / 128.0


def moments(X, mean, s, r):
    """Generic inputs -> (H, g in 80-bit sums of the float64 terms the definition names, |terms| summed: Ha, ga).  The
    terms: a = s_i * u~_ia (one rounding), then a * u~_ib."""
    ut = _tilde(X, mean, np.float64)
    a = np.asarray(s, np.float64)[:, None] * ut
    H = (a.astype(LD).T @ ut.astype(LD)).astype(np.float64)
    Ha = (np.abs(a).astype(LD).T @ np.abs(ut).astype(LD)).astype(np.float64)
    rl = np.asarray(r, np.float64).astype(LD)
    g = (ut.astype(LD).T @ rl).astype(np.float64)
    ga = (np.abs(ut).astype(LD).T @ np.abs(rl)).astype(np.float64)
    return H, g, Ha, ga


def moment_bound(n, ab):
    """|moment - reference| allowed: (n + 8) 2^-53 x the sum of the absolute terms (the form and the reasoning of
    chain_ref.moment_bound: any order of n terms, the second product formed inside a fused multiply-add, the 80-bit
    reference's own rounding, second order)."""
    return (n + 8.0) * U * ab


# ---------------------------------------------------------------------------------- the 80-bit Newton
def objective(ut, y, beta, C):
    z = ut @ beta
    return (np.maximum(z, 0) - np.where(y, z, 0) + np.log1p(np.exp(-np.abs(z)))).sum() + (beta[:-1] ** 2).sum() / (2 * LD(C))


def newton(X, y, C=1.0, iters=200):
    """The minimiser of sum log(1 + e^z) - y z + ||w||^2 / (2 C) in 80-bit arithmetic, textbook form: features centred
    by their 80-bit mean, Newton steps by Gaussian elimination, a step above 1e-6 halved while the objective rises, until a
    step no longer moves any coefficient by 1e-17 -> (w [D], b for the uncentred x), float64."""
    Xl = np.asarray(X, F32).astype(LD)
    mu = Xl.sum(0) / LD(Xl.shape[0])
    ut = np.concatenate([Xl - mu[None, :], np.ones((Xl.shape[0], 1), LD)], axis=1)
    yb = np.asarray(y) != 0
    m = ut.shape[1]
    ybar = LD(yb.mean())
    beta = np.zeros(m, LD)
    beta[-1] = np.log(ybar / (1 - ybar))
    ridge = np.ones(m, LD) / LD(C)
    ridge[-1] = 0
    F = objective(ut, yb, beta, C)
    for _ in range(iters):
        z = ut @ beta
        e = np.exp(-np.abs(z))
        p = np.where(z >= 0, 1 / (1 + e), e / (1 + e))
        q = np.where(z >= 0, e / (1 + e), 1 / (1 + e))
        g = ut.T @ np.where(yb, -q, p) + ridge * beta
        H = (ut * (p * q)[:, None]).T @ ut + np.diag(ridge)
        step = _solve(H, g)
        scale = LD(1)
        while True:
            new = beta - scale * step
            Fn = objective(ut, yb, new, C)
            if Fn <= F or np.abs(scale * step).max() < 1e-6:          # a small step is Newton's own: F moves by rounding only
                break
            scale = scale / 2
        moved = np.abs(new - beta).max()
        beta, F = new, Fn
        if moved < 1e-17:
            break
    w = beta[:-1]
    return w.astype(np.float64), np.float64(beta[-1] - (w * mu).sum())


def _solve(A, b):
    """Gaussian elimination with partial pivoting in the dtype of A (numpy.linalg has no 80-bit path)."""
    A, b = A.copy(), b.copy()
    m = b.size
    for k in range(m):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
            b[[k, piv]] = b[[piv, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= f[:, None] * A[k, k:][None, :]
        b[k + 1:] -= f * b[k]
    x = np.zeros(m, A.dtype)
    for k in range(m - 1, -1, -1):
        x[k] = (b[k] - (A[k, k + 1:] * x[k + 1:]).sum()) / A[k, k]
    return x


# ---------------------------------------------------------------------------------- weighted error sums over pairs
def pair_case(m, n, L, seed, order="shuffled", empty_lab=None):
    """-> (pred, target fp32 [m], patient, lab int64 [m], P fp32 [n, L] with cells under the clip and at 1, cov fp64 [L])."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, L, m)
    if empty_lab is not None and L > 1:
        lab[lab == empty_lab] = (empty_lab + 1) % L
    if order == "lab-major":
        lab = np.sort(lab, kind="stable")
    patient = rng.integers(0, n, m)
    P = rng.random((n, L)).astype(F32)
    P[rng.random((n, L)) < 0.1] = F32(0.001)
    P[rng.random((n, L)) < 0.05] = F32(1.0)
    target = rng.standard_normal(m).astype(F32)
    pred = (target + rng.standard_normal(m) * 0.5).astype(F32)
    return pred, target, patient.astype(np.int64), lab.astype(np.int64), P, rng.random(L) * 0.9 + 0.05


def pair_sums(pred, target, patient, lab, P, cov, clip, stabilized):
    """Loops in 80-bit arithmetic -> (count [L + 1], sums [L + 1, 6] as longdouble): n, sum w, w^2, w |e|, w e^2, |e|,
    e^2 per lab and, in the last row, over all pairs."""
    n, L = P.shape
    count, sums = np.zeros(L + 1, np.int64), np.zeros((L + 1, 6), LD)
    for i in range(len(pred)):
        j = int(lab[i])
        e = LD(pred[i]) - LD(target[i])
        w = (LD(cov[j]) if stabilized else LD(1)) / max(LD(P[int(patient[i]), j]), LD(clip))
        terms = np.array([w, w * w, w * abs(e), w * e * e, abs(e), e * e], LD)
        for row in (j, L):
            count[row] += 1
            sums[row] += terms
    return count, sums


def pair_bound(count, sums):
    """|sum - reference| allowed: (n + 8) 2^-53 x the sum (every term is >= 0 and carries at most three roundings; n
    additions in any order)."""
    return (count[:, None] + 8.0) * U * sums.astype(np.float64)


CASES = [(kind, n, D) for kind in ("generic", "rare", "separable") for n, D in ((300, 3), (2000, 17), (2000, 64), (500, 128))]
