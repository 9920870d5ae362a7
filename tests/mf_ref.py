"""Loop reference of lab imputation by low-rank matrix completion (mmgnn/lowrank.py, csrc/mf.hip): the normal
equations of one segment by math.fsum (the correctly rounded sum of its float64 terms), the solve and the whole
alternating chain -- centres, normal equations, Cholesky, rounds, closing half-sweep -- in 80-bit numpy.longdouble, row
by row; the sum rule of include/mmgnn_mf.h restated with numpy's sequential cumsum.  Independent of the numpy
restatement.  Also the test inputs: segment lists of chosen lengths, on a lattice (multiples of 1/8 of small magnitude,
so that every sum is exact in fp64) or generic, and random triples."""
import math

import numpy as np

F32 = np.float32
LD = np.longdouble
U = 2.0 ** -53
CHUNK = 256                           # MMG_MF_CHUNK (the tests assert it against the header)


# ---------------------------------------------------------------------------------- inputs
def make_segments(lengths, m, r, seed=0, lattice=False):
    """-> (ptr int64 [S + 1], idx int32 [nnz], y fp64 [nnz], F fp64 [m, r]): segments of the given lengths, in order.
    Lattice: F and y are multiples of 1/8 in [-1, 1]: every product is a multiple of 1/64 below 1 and every sum of
    fewer than 2^40 of them is exact."""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int64)
    nnz = int(ptr[-1])
    idx = rng.integers(0, m, nnz).astype(np.int32)
    if lattice:
        F = rng.integers(-8, 9, (m, r)) / 8.0
        y = rng.integers(-8, 9, nnz) / 8.0
    else:
        F = rng.standard_normal((m, r))
        y = rng.standard_normal(nnz) * 2.0 + 0.3
    return ptr, idx, np.ascontiguousarray(y, np.float64), np.ascontiguousarray(F, np.float64)


def make_triples(n, L, density=0.3, seed=0, lattice=False, empty_lab=None):
    """-> (patient int64, lab int64, value fp32) in random order, every pair at most once; ``empty_lab`` has none."""
    rng = np.random.default_rng(seed)
    mask = rng.random((n, L)) < density
    if empty_lab is not None:
        mask[:, empty_lab] = False
    p, lab = np.nonzero(mask)
    if lattice:
        v = rng.integers(-16, 17, p.size) / 8.0
    else:
        rows, cols = rng.standard_normal((n, 3)), rng.standard_normal((L, 3))
        v = (rows[p] * cols[lab]).sum(1) + 0.3 * rng.standard_normal(p.size) + 0.5 * lab
    order = rng.permutation(p.size)
    return p[order].astype(np.int64), lab[order].astype(np.int64), v[order].astype(F32)


# ---------------------------------------------------------------------------------- the sum rule
def serial(x) -> float:
    """The items added one after the other, ascending, onto 0."""
    x = np.asarray(x, np.float64)
    return float(np.cumsum(x)[-1]) if x.size else 0.0


def chunk_sums(x) -> np.ndarray:
    x = np.asarray(x, np.float64)
    return np.array([serial(x[c:c + CHUNK]) for c in range(0, x.size, CHUNK)])


def rule_sum(x) -> float:
    """One segment under the rule: its chunk sums, added one after the other in ascending order."""
    return serial(chunk_sums(x))


def rule_sum_levels(x) -> float:
    """The objective's form: the chunk sums themselves summed by the rule, level after level, until one is left."""
    x = np.asarray(x, np.float64)
    if x.size == 0:
        return 0.0
    while True:
        x = chunk_sums(x)
        if x.size == 1:
            return float(x[0])


# ---------------------------------------------------------------------------------- one half-sweep, term by term
def normal(ptr, idx, y, F, reg):
    """-> (A [S, r, r], b [S, r] by fsum; Aa, ba: the sums of the absolute values of the same terms).  The terms are
    the float64 products f_k f_l and f_k y (one rounding each) and, on the diagonal, reg."""
    S, r = len(ptr) - 1, F.shape[1]
    A, Aa = np.zeros((S, r, r)), np.zeros((S, r, r))
    b, ba = np.zeros((S, r)), np.zeros((S, r))
    for s in range(S):
        q = slice(int(ptr[s]), int(ptr[s + 1]))
        f, ys = F[np.asarray(idx[q], np.int64)], y[q]
        for k in range(r):
            for l in range(k + 1):
                prod = f[:, k] * f[:, l]
                if k == l:
                    prod = np.append(prod, np.float64(reg))
                A[s, k, l] = A[s, l, k] = math.fsum(prod.tolist())
                Aa[s, k, l] = Aa[s, l, k] = math.fsum(np.abs(prod).tolist())
            prod = f[:, k] * ys
            b[s, k], ba[s, k] = math.fsum(prod.tolist()), math.fsum(np.abs(prod).tolist())
    return A, b, Aa, ba


def sum_bound(length, ab):
    """|sum - fsum| allowed: (length + 8) 2^-53 x the sum of the absolute terms -- any order of the terms, a product
    formed inside a fused multiply-add, the one addition of reg, second order (the form of chain_ref.moment_bound)."""
    return (np.asarray(length, np.float64) + 8.0) * U * ab


def solve_ld(A, b):
    """A x = b for a symmetric positive definite A, 80-bit, row by row (Cholesky-Banachiewicz)."""
    A, b = np.asarray(A, LD), np.asarray(b, LD)
    m = b.size
    Lo = np.zeros((m, m), LD)
    for i in range(m):
        for k in range(i):
            Lo[i, k] = (A[i, k] - np.dot(Lo[i, :k], Lo[k, :k])) / Lo[k, k]
        Lo[i, i] = np.sqrt(A[i, i] - np.dot(Lo[i, :i], Lo[i, :i]))
    z = np.zeros(m, LD)
    for i in range(m):
        z[i] = (b[i] - np.dot(Lo[i, :i], z[:i])) / Lo[i, i]
    x = np.zeros(m, LD)
    for i in range(m - 1, -1, -1):
        x[i] = (z[i] - np.dot(Lo[i + 1:, i], x[i + 1:])) / Lo[i, i]
    return x


# ---------------------------------------------------------------------------------- the whole chain, 80-bit
def _half_ld(groups, other, reg, r):
    out = np.zeros((len(groups), r), LD)
    eye = LD(reg) * np.eye(r, dtype=LD)
    for s, (ids, ys) in enumerate(groups):
        if len(ids):
            f = other[ids]
            out[s] = solve_ld(f.T @ f + eye, f.T @ ys)
    return out


def als(patient, lab, value, n_patients, n_labs, V0, reg, rounds, center=None):
    """-> (U, V longdouble, the objective F after every round, center): ``rounds`` rounds from V0 and the closing patient
    half-sweep, all in 80-bit arithmetic, from the triples in the order given (no ordering, no chunks)."""
    assert np.finfo(LD).nmant >= 63, "no 80-bit long double on this platform"
    p, lb = np.asarray(patient, np.int64), np.asarray(lab, np.int64)
    v = np.asarray(value, F32).astype(LD)
    r = V0.shape[1]
    if center is None:
        center = np.zeros(n_labs, LD)
        for l in range(n_labs):
            if (lb == l).any():
                center[l] = v[lb == l].sum() / LD(int((lb == l).sum()))
    center = np.asarray(center, LD)
    y = v - center[lb]
    by_p = [(lb[p == i], y[p == i]) for i in range(n_patients)]
    by_l = [(p[lb == l], y[lb == l]) for l in range(n_labs)]
    V = np.asarray(V0, np.float64).astype(LD)
    V[[l for l in range(n_labs) if not len(by_l[l][0])]] = 0
    hist = []
    for _ in range(rounds):
        Uf = _half_ld(by_p, V, reg, r)
        V = _half_ld(by_l, Uf, reg, r)
        d = y - (Uf[p] * V[lb]).sum(1)
        hist.append(float((d * d).sum() + LD(reg) * ((Uf * Uf).sum() + (V * V).sum())))
    Uf = _half_ld(by_p, V, reg, r)
    return Uf, V, hist, center
