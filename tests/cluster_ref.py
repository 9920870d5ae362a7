"""An independent float64 restatement of include/mmgnn_cluster.h for the tests: plain loops over rows and clusters, no
import of the package.  Distances in the difference form from the widened fp32 rows, columns ascending; the key (s, c)
with ties to the smaller centre; sums in ascending row order; the e-th empty cluster (ascending index) takes the row with
the e-th largest key (min_s descending, smaller row first)."""
import numpy as np


def blobs(n, D, k, seed, spread=4.0):
    """n fp32 rows around k Gaussian centres."""
    rs = np.random.RandomState(seed)
    c = rs.randn(k, D) * spread
    return (c[rs.randint(k, size=n)] + rs.randn(n, D)).astype(np.float32)


def lattice(n, D, seed, span=3):
    """Small integers: every sum is exact in either arithmetic and ties are real."""
    return np.random.RandomState(seed).randint(-span, span + 1, size=(n, D)).astype(np.float32)


def init_rows(x, k, seed=1):
    return x[np.random.RandomState(seed).choice(x.shape[0], k, replace=False)].astype(np.float64)


def sqdist(x, centers):
    x64, c64 = x.astype(np.float32).astype(np.float64), np.asarray(centers, np.float64)
    s = np.zeros((x64.shape[0], c64.shape[0]))
    for d in range(x64.shape[1]):
        s = s + (x64[:, d][:, None] - c64[:, d][None, :]) ** 2
    s[~np.isfinite(s)] = np.inf
    return s


def assign(x, centers):
    s = sqdist(x, centers)
    labels = np.zeros(x.shape[0], np.int32)
    for i in range(x.shape[0]):
        best = 0
        for c in range(1, s.shape[1]):
            if s[i, c] < s[i, best]:
                best = c
        labels[i] = best
    return labels, s[np.arange(x.shape[0]), labels]


def update(x, labels, min_s, old):
    x64 = x.astype(np.float32).astype(np.float64)
    k = old.shape[0]
    sums, counts = np.zeros_like(old), np.zeros(k, np.int64)
    for i in range(x64.shape[0]):
        sums[labels[i]] = sums[labels[i]] + x64[i]
        counts[labels[i]] += 1
    empty = [c for c in range(k) if counts[c] == 0]
    order = sorted(range(x64.shape[0]), key=lambda i: (-min_s[i], i))
    rows = order[:len(empty)]
    for c, row in zip(empty, rows):
        sums[labels[row]] = sums[labels[row]] - x64[row]
        counts[labels[row]] -= 1
        sums[c] = sums[c] + x64[row]
        counts[c] = 1
    new = np.array(old, np.float64)
    shift = 0.0
    for c in range(k):
        if counts[c] > 0:
            new[c] = sums[c] / float(counts[c])
        t = 0.0
        for d in range(old.shape[1]):
            t += (new[c, d] - old[c, d]) ** 2
        shift += t
    return new, counts, shift, len(empty), np.array(rows, np.int64)


def kmeans(x, init, max_iter=300, tol=1e-4):
    """-> (centres, labels, inertia, n_iter, counts of the final labels, min_s)."""
    centers = np.array(init, np.float64)
    tol_abs = float(np.mean(np.var(x.astype(np.float64), axis=0))) * tol
    old_labels, strict, n_iter = None, False, 0
    for it in range(max_iter):
        labels, min_s = assign(x, centers)
        centers, _, shift, _, _ = update(x, labels, min_s, centers)
        n_iter = it + 1
        if old_labels is not None and np.array_equal(labels, old_labels):
            strict = True
            break
        if shift <= tol_abs:
            break
        old_labels = labels
    if not strict:
        labels, min_s = assign(x, centers)
    inertia = 0.0
    for v in min_s:
        inertia += v
    return centers, labels, inertia, n_iter, np.bincount(labels, minlength=centers.shape[0]), min_s


def silhouette(x, labels, queries=None):
    x64 = x.astype(np.float32).astype(np.float64)
    n, k = x64.shape[0], int(labels.max()) + 1
    counts = np.bincount(labels, minlength=k)
    q = range(n) if queries is None else queries
    out = []
    for i in q:
        df = x64 - x64[i]
        s = np.zeros(n)
        for d in range(x64.shape[1]):
            s = s + df[:, d] ** 2
        r = np.sqrt(s)
        r[i] = 0.0
        S = np.array([r[labels == c].sum() for c in range(k)])
        own = labels[i]
        if counts[own] <= 1:
            out.append(0.0)
            continue
        a = S[own] / (counts[own] - 1)
        b = min(S[c] / counts[c] for c in range(k) if c != own and counts[c] > 0)
        out.append((b - a) / max(a, b) if max(a, b) > 0 else 0.0)
    return np.array(out)
