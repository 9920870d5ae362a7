"""The host checker of the neighbour tests (test_neighbors_cpu.py, test_neighbors_gpu.py): an independent float64
restatement of the contract in include/mmgnn_nn.h -- s(q, j) = sum_d (q_d - x_jd)^2 from the widened fp32 inputs, columns in
ascending order; candidates ordered by np.lexsort on (index, s), a non-finite sum as +inf; self mode drops j == q -- and
the input generators with the precondition the generic inputs are held to."""
import numpy as np

MIN_GAP = 1e-10              # smallest relative gap between consecutive sorted distances a generic input may have
GENERIC_SHAPES = [(300, 16), (257, 128), (130, 4), (1000, 128)]


def lattice(n, D, seed=5, span=3):
    """Small integers (-span .. span) as fp32: every sum is exact in fp64, so device, host and fma agree bit for bit, and
    real ties (and, at span 3, duplicate rows) occur."""
    return np.random.default_rng(seed).integers(-span, span + 1, size=(n, D)).astype(np.float32)


def generic(n, D, seed=0):
    return np.random.default_rng(seed).normal(size=(n, D)).astype(np.float32)


def sums(q, x):
    """float64 [nq, n]: columns ascending, one product and one addition per column."""
    q64, x64 = q.astype(np.float64), x.astype(np.float64)
    s = np.zeros((q.shape[0], x.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(x.shape[1]):
            df = q64[:, d][:, None] - x64[:, d][None, :]
            s = s + df * df
    return np.where(np.isfinite(s), s, np.inf)


def full_order(x, rows=None, queries=None):
    """-> (order int64 [r, n or n - 1], the sums in that order): every candidate of the query rows in ascending key
    order.  queries None: self mode over the rows `rows` (default all) of x, j == q dropped."""
    n = x.shape[0]
    if queries is None:
        rows = np.arange(n) if rows is None else np.asarray(rows)
        q = x[rows]
    else:
        q = queries
    s = sums(q, x)
    idx = np.broadcast_to(np.arange(n), s.shape)
    order = np.lexsort((idx, s), axis=-1)
    if queries is None:
        order = order[order != rows[:, None]].reshape(len(rows), n - 1)
    return order, np.take_along_axis(s, order, axis=1)


def knn(x, k, rows=None, queries=None):
    """-> (indices int64 [r, k], distances fp32 [r, k] = the float64 root rounded once)."""
    order, s = full_order(x, rows, queries)
    return order[:, :k].copy(), np.sqrt(s[:, :k]).astype(np.float32)


def ranks(x, nbr, rows=None):
    """rank(i, nbr[i, c]) for the rows `rows` (default all): 1-based position in the full order, 0 for an invalid
    entry (negative, >= n, or i itself) -> int32 [r, k]."""
    n = x.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    order, _ = full_order(x, rows)
    out = np.zeros((len(rows), nbr.shape[1]), np.int32)
    for a, i in enumerate(rows):
        pos = np.zeros(n, np.int32)
        pos[order[a]] = np.arange(1, n)
        for c, j in enumerate(nbr[i]):
            if 0 <= j < n and j != i:
                out[a, c] = pos[j]
    return out


def penalty(x, nbr):
    k = nbr.shape[1]
    return int(np.maximum(ranks(x, nbr).astype(np.int64) - k, 0).sum())


def trustworthiness(x, y, k):
    n = x.shape[0]
    return 1.0 - penalty(x, knn(y, k)[0]) * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


def min_relative_gap(x, queries=None):
    """The smallest (d[c + 1] - d[c]) / d[c + 1] over consecutive sorted distances of any row: what a generic input is
    asserted on before equality of indices is asked of it."""
    _, s = full_order(x, queries=queries)
    d = np.sqrt(s)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (d[:, 1:] - d[:, :-1]) / d[:, 1:]
    return float(np.nanmin(gap))


def ulp_diff(got, want):
    """|got - want| in units of the fp32 spacing at want."""
    want = want.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.float32(1e-30)))
