"""K-means cohorts of the node embeddings and their scores: ``sklearn.cluster.KMeans(algorithm="lloyd")`` semantics with
``davies_bouldin_score``, ``calinski_harabasz_score`` and ``silhouette_samples``, without an n x n matrix
(``csrc/cluster.hip``: ``mmg_km_assign``, ``mmg_km_update``, ``mmg_km_scores``, ``mmg_km_silhouette``).

The result is defined by total orders and stated orders of summation (``include/mmgnn_cluster.h``): the squared distance
``s(i, c) = sum_d (x_id - C_cd)^2`` is taken in the difference form in float64 from the fp32 rows, columns ascending; a row
goes to the centre with the smallest key ``(s, c)`` -- equal sums to the smaller centre index; the e-th empty cluster (in
ascending index) takes the row with the e-th largest key (``min_s`` descending, then the smaller row), which leaves the
sum and count of its own cluster; a cluster left with no row keeps its centre.  The loop is sklearn's
``_kmeans_single_lloyd``: stop when no label changed (strict), or when the squared centre shift is at most
``mean_d(var_d(x)) * tol``, after which the rows are assigned once more against the final centres.  sklearn's
mean-centring of x is a conditioning step for its Gram-form distance; the difference form does not need it.
``inertia`` is the sum of the last assignment's ``min_s`` (after a strict stop with an empty cluster the relocated
centres are returned as sklearn returns them, while ``inertia`` stays that of the assignment they were made from).

A HIP fp32 tensor runs the kernels and the arrays stay on the device.  A numpy array (or host tensor) runs the float64
restatement below: that path is the checker and the only one without a GPU.  Only the Euclidean metric is offered.
"""
from __future__ import annotations

import logging
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import pandas as pd
import torch

from . import cluster_ops, embed, neighbors
from .data import LAB_EDGE

MAX_K = cluster_ops.KM_MAX_K     # read from include/mmgnn_cluster.h by the binding (the library itself is not loaded for it)
MAX_D = cluster_ops.KM_MAX_D
KMEANSPP_MAX_ROWS = 16384        # k-means++ draws its centres from a seeded sample of at most this many rows
SWEEP_COLUMNS = ["k", "inertia", "davies_bouldin", "calinski_harabasz", "silhouette", "n_iter", "smallest_cluster"]
PATIENT_CLUSTER_COLUMNS = ["patient_id", "cluster", "distance"]
CLUSTER_SUMMARY_COLUMNS = ["cluster", "n_patients", "mean_lab_degree", "median_lab_degree", "mean_distance",
                           "silhouette_mean"]
LAB_PROFILE_COLUMNS = ["cluster", "lab_idx", "lab_name", "n_observed", "coverage", "mean_value", "std_value"]
LAB_CLUSTER_COLUMNS = ["lab_idx", "lab_name", "panel", "cluster", "distance"]


@dataclass
class KMeansResult:
    cluster_centers: object                  # fp64 [k, D]: device tensor, or numpy on the host path
    labels: object                           # int32 [n]
    inertia: float
    n_iter: int
    counts: object                           # int32 [k]: the rows per label
    converged: bool                          # stopped by either rule before max_iter ran out
    sqdist: object = None                    # fp64 [n]: every row's squared distance to its centre
    sdist: object = None                     # fp64 [k]: per cluster the sum of the rows' distances to its centre
    min_gap: float = float("inf")            # host path: the smallest relative gap between a row's two best keys


def _rows(x, name: str):
    """-> (a device fp32 tensor or a host fp32 numpy array [n, D], on the device?)."""
    if embed._is_dev(x):
        x = x.detach()
        if x.dtype != torch.float32:
            raise TypeError(f"{name}: expected torch.float32 on the device, got {x.dtype}")
        if x.dim() == 2 and int(x.shape[1]) > 1 and x.stride(1) != 1:
            x = x.contiguous()
        dev = True
    else:
        x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
        if x.dtype.kind != "f":
            raise TypeError(f"{name}: expected a floating-point array, got {x.dtype}")
        x = x.astype(np.float32)
        dev = False
    if x.ndim != 2:
        raise ValueError(f"{name}: expected [n, D] rows, got {x.ndim} dimensions")
    if not 1 <= int(x.shape[1]) <= MAX_D:
        raise ValueError(f"{name}: D = {int(x.shape[1])} outside [1, {MAX_D}]")
    if int(x.shape[0]) < 1:
        raise ValueError(f"{name}: no rows")
    return x, dev


def _check_k(k, n: int, what: str, lo: int = 1) -> int:
    k = int(k)
    if not lo <= k <= MAX_K:
        raise ValueError(f"{what}: n_clusters = {k} outside [{lo}, {MAX_K}]")
    if k > n:
        raise ValueError(f"{what}: n_clusters = {k} exceeds the {n} rows")
    return k


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


# ---------------------------------------------------------------------------- the float64 host restatement
def sqdist_host(x, centers) -> np.ndarray:
    """s[i, c] = sum_d (x[i, d] - centers[c, d])^2 in float64, x widened from fp32, columns in ascending order; a
    non-finite sum is +inf."""
    x64, c64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(centers, np.float64)
    s = np.zeros((x64.shape[0], c64.shape[0]), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(x64.shape[1]):
            df = x64[:, d:d + 1] - c64[None, :, d]
            s += df * df
    s[~np.isfinite(s)] = np.inf
    return s


def assign_host(x, centers):
    """-> (labels int32 [n], min_s fp64 [n], the smallest relative gap (second - best) / second over the rows; inf for
    one centre)."""
    n, k = int(np.shape(x)[0]), int(np.shape(centers)[0])
    labels, min_s, gap = np.empty(n, np.int32), np.empty(n, np.float64), np.inf
    for a, b in neighbors._host_blocks(n, k * 4):
        s = sqdist_host(x[a:b], centers)
        lab = np.argmin(s, axis=1)                                # the first minimum: the smaller centre index
        labels[a:b] = lab
        min_s[a:b] = s[np.arange(b - a), lab]
        if k > 1:
            two = np.partition(s, 1, axis=1)[:, :2]
            ok = np.isfinite(two[:, 1]) & (two[:, 1] > 0)
            if ok.any():
                gap = min(gap, float(((two[ok, 1] - two[ok, 0]) / two[ok, 1]).min()))
            if (~ok & (two[:, 1] == two[:, 0])).any():
                gap = 0.0
    return labels, min_s, gap


def update_host(x, labels, min_s, centers_old):
    """One centre update (module docstring; sums in ascending row order) -> (centers_new fp64 [k, D], counts int64 [k]
    after relocation, shift, m = the empty clusters, the rows they took int64 [m])."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    old = np.asarray(centers_old, np.float64)
    k = old.shape[0]
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    sums = np.zeros_like(old)
    np.add.at(sums, labels, x64)
    empty = np.flatnonzero(counts == 0)
    rows = np.argsort(-np.asarray(min_s, np.float64), kind="stable")[:empty.size].astype(np.int64)
    for c, row in zip(empty, rows):
        sums[labels[row]] -= x64[row]
        counts[labels[row]] -= 1
        sums[c] += x64[row]
        counts[c] = 1
    new = old.copy()
    live = counts > 0
    new[live] = sums[live] / counts[live, None].astype(np.float64)
    shift = 0.0
    for c in range(k):
        t = 0.0
        for v in (new[c] - old[c]) ** 2:
            t += v
        shift += t
    return new, counts, float(shift), int(empty.size), rows


def scores_host(labels, min_s, k: int):
    """-> (inertia, sdist fp64 [k], counts int64 [k]) in ascending row order."""
    min_s = np.asarray(min_s, np.float64)
    sdist = np.zeros(k, np.float64)
    np.add.at(sdist, labels, np.sqrt(min_s))
    return float(np.add.accumulate(min_s)[-1]), sdist, np.bincount(labels, minlength=k).astype(np.int64)


def kmeans_host(x, centers, max_iter: int, tol: float) -> KMeansResult:
    x = np.asarray(x, np.float32)
    centers = np.array(centers, np.float64)
    k = centers.shape[0]
    tol_abs = float(np.mean(np.var(x.astype(np.float64), axis=0))) * tol
    labels_old, gap, strict, converged, n_iter = None, np.inf, False, False, 0
    for it in range(max_iter):
        labels, min_s, g = assign_host(x, centers)
        gap = min(gap, g)
        centers, _, shift, _, _ = update_host(x, labels, min_s, centers)
        n_iter = it + 1
        if labels_old is not None and np.array_equal(labels, labels_old):
            strict = converged = True
            break
        if shift <= tol_abs:
            converged = True
            break
        labels_old = labels
    if not strict:
        labels, min_s, g = assign_host(x, centers)
        gap = min(gap, g)
    inertia, sdist, counts = scores_host(labels, min_s, k)
    return KMeansResult(centers, labels, inertia, n_iter, counts.astype(np.int32), converged, min_s, sdist, float(gap))


def silhouette_samples_host(x, labels, queries=None) -> np.ndarray:
    """The silhouette coefficients in float64; S(i, c) sums the candidates of cluster c per row on its own (the rows
    sorted by label, one segment sum per cluster), so a row's value does not depend on which other rows are asked for."""
    x = np.asarray(x, np.float32)
    labels = np.asarray(labels, np.int64)
    n, k = x.shape[0], int(labels.max()) + 1
    counts = np.bincount(labels, minlength=k).astype(np.float64)
    order = np.argsort(labels, kind="stable")
    live = np.flatnonzero(counts > 0)
    starts = np.concatenate([[0], np.cumsum(counts[live]).astype(np.int64)[:-1]])
    q = np.arange(n, dtype=np.int64) if queries is None else np.asarray(queries, np.int64)
    out = np.zeros(q.size, np.float64)
    for a, b in neighbors._host_blocks(q.size, n):
        rows = q[a:b]
        r = np.sqrt(neighbors.sqdist_host(x[rows], x))
        r[np.arange(b - a), rows] = 0.0
        S = np.full((b - a, k), np.inf)
        S[:, live] = np.add.reduceat(r[:, order], starts, axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            own = labels[rows]
            cn = counts[own]
            a_ = S[np.arange(b - a), own] / (cn - 1.0)
            other = S / counts[None, :]
            other[np.arange(b - a), own] = np.inf
            other[:, counts == 0] = np.inf
            b_ = other.min(axis=1)
            den = np.maximum(a_, b_)
            v = (b_ - a_) / den
        v[(cn <= 1) | ~(den > 0) | ~np.isfinite(den)] = 0.0
        out[a:b] = v
    return out


# ---------------------------------------------------------------------------- k-means++ (host, float64)
def kmeans_plusplus(x, n_clusters: int, seed: int = 0) -> np.ndarray:
    """sklearn's greedy k-means++ recipe (``_kmeans_plusplus``: ``2 + int(log k)`` local trials per centre, the
    candidate with the lowest potential kept) in float64 on the host, over a sample of at most ``KMEANSPP_MAX_ROWS`` rows
    drawn without replacement by ``numpy.random.RandomState(seed)`` (all rows when there are no more).  The same recipe
    as sklearn's, NOT sklearn's draw: sklearn draws from every row with its own stream of random numbers, which would have
    to be restated bit for bit to be checkable.  -> centres fp64 [k, D] (rows of x, widened)."""
    rs = np.random.RandomState(seed)
    n = int(x.shape[0])
    if n > KMEANSPP_MAX_ROWS:
        pick = np.sort(rs.choice(n, KMEANSPP_MAX_ROWS, replace=False))
        xs = x[torch.from_numpy(pick).to(x.device)] if torch.is_tensor(x) else x[pick]
    else:
        xs = x
    xs = _host(xs).astype(np.float64)
    n, k = xs.shape[0], int(n_clusters)
    trials = 2 + int(math.log(k))
    centers = np.empty((k, xs.shape[1]), np.float64)
    centers[0] = xs[rs.randint(n)]
    closest = ((xs - centers[0]) ** 2).sum(axis=1)
    pot = float(closest.sum())
    for c in range(1, k):
        cand = np.searchsorted(np.cumsum(closest), rs.uniform(size=trials) * pot)
        np.clip(cand, None, n - 1, out=cand)
        d = ((xs[cand][:, None, :] - xs[None, :, :]) ** 2).sum(axis=2)
        np.minimum(closest, d, out=d)
        pots = d.sum(axis=1)
        best = int(np.argmin(pots))
        pot, closest, centers[c] = float(pots[best]), d[best], xs[cand[best]]
    return centers


# ---------------------------------------------------------------------------- the public calls
def _kmeans_dev(x, centers, max_iter: int, tol: float) -> KMeansResult:
    ops = cluster_ops
    n, k = int(x.shape[0]), int(centers.shape[0])
    dev = x.device
    centers = centers.clone()
    tol_abs = float(ops.km_colstats(x)[1].item()) * tol
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    min_s = torch.empty(n, dtype=torch.float64, device=dev)
    changed = torch.empty(1, dtype=torch.int64, device=dev)
    counts = torch.empty(k, dtype=torch.int32, device=dev)
    status = torch.empty(3, dtype=torch.float64, device=dev)
    strict, converged, n_iter = False, False, 0
    for it in range(max_iter):
        ops.km_assign(x, centers, labels if it else None, labels, min_s, changed)
        ops.km_update(x, labels, min_s, centers, centers, counts, changed, status)
        n_changed, shift, _ = status.tolist()                    # the one read of the iteration
        n_iter = it + 1
        if n_changed == 0:
            strict = converged = True
            break
        if shift <= tol_abs:
            converged = True
            break
    if not strict:
        ops.km_assign(x, centers, None, labels, min_s, None)
    inertia, sdist, counts = ops.km_scores(labels, min_s, k)
    return KMeansResult(centers, labels, float(inertia.item()), n_iter, counts, converged, min_s, sdist)


def kmeans(x, n_clusters: int, init="k-means++", n_init: int = 1, max_iter: int = 300, tol: float = 1e-4,
           seed: int = 0) -> KMeansResult:
    """``sklearn.cluster.KMeans(n_clusters, init=..., n_init=..., max_iter=..., tol=..., algorithm="lloyd")`` over the rows
    ``x`` [n, D] (module docstring).  ``init``: an array [k, D] of starting centres (one run, ``n_init`` must be 1), or
    ``"k-means++"``: ``kmeans_plusplus`` with seeds ``seed, seed + 1, ...`` for the ``n_init`` runs, of which the one with
    the lowest inertia is kept (ties: the earlier run).  ``1 <= n_clusters <= MAX_K`` (128), ``n_clusters <= n``,
    ``1 <= D <= MAX_D`` (256).  -> ``KMeansResult(cluster_centers fp64 [k, D], labels int32 [n], inertia, n_iter, counts,
    converged)``."""
    x, dev = _rows(x, "x")
    n, D = int(x.shape[0]), int(x.shape[1])
    k = _check_k(n_clusters, n, "kmeans")
    if int(max_iter) < 1 or int(n_init) < 1:
        raise ValueError(f"kmeans: max_iter = {max_iter} and n_init = {n_init} must be at least 1")
    if isinstance(init, str):
        if init != "k-means++":
            raise ValueError(f'kmeans: init must be "k-means++" or an array [{k}, {D}], got {init!r} (a random draw of '
                             "rows is sklearn's own stream of random numbers and is not restated)")
        starts = [None] * int(n_init)
    else:
        c0 = _host(init)
        if c0.dtype.kind != "f":
            raise TypeError(f"kmeans: init must be a floating-point array, got {c0.dtype}")
        if c0.shape != (k, D):
            raise ValueError(f"kmeans: init has shape {tuple(c0.shape)}, expected ({k}, {D})")
        if int(n_init) != 1:
            raise ValueError("kmeans: an explicit init is one run: n_init must be 1")
        starts = [c0.astype(np.float64)]
    best = None
    for r, c0 in enumerate(starts):
        if c0 is None:
            c0 = kmeans_plusplus(x, k, int(seed) + r)
        if dev:
            res = _kmeans_dev(x, torch.from_numpy(np.ascontiguousarray(c0)).to(x.device), int(max_iter), float(tol))
        else:
            res = kmeans_host(x, c0, int(max_iter), float(tol))
        if best is None or res.inertia < best.inertia:
            best = res
    return best


def assign(x, centers):
    """Every row's nearest centre under the key (s, c) -> ``(labels int32 [n], sqdist fp64 [n])``."""
    x, dev = _rows(x, "x")
    c = _host(centers) if not (dev and embed._is_dev(centers)) else centers
    if tuple(c.shape) != (int(c.shape[0]), int(x.shape[1])) or c.ndim != 2:
        raise ValueError(f"assign: centers has shape {tuple(c.shape)}, expected (k, {int(x.shape[1])})")
    _check_k(int(c.shape[0]), int(x.shape[0]), "assign")
    if dev:
        c = c.to(torch.float64).contiguous() if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c, np.float64)).to(x.device)
        return cluster_ops.km_assign(x, c)
    labels, min_s, _ = assign_host(x, np.asarray(c, np.float64))
    return labels, min_s


def _compact(labels, n: int, dev: bool, device=None):
    """sklearn's LabelEncoder: the labels renumbered 0 .. k - 1 in ascending order of their values -> (int32 labels, k)."""
    lab = _host(labels).reshape(-1)
    if lab.size != n:
        raise ValueError(f"labels has {lab.size} entries for {n} rows")
    if lab.dtype.kind not in "iu":
        raise TypeError(f"labels: expected integers, got {lab.dtype}")
    uniq, inv = np.unique(lab, return_inverse=True)
    inv = inv.astype(np.int32)
    return (torch.from_numpy(inv).to(device) if dev else inv), int(uniq.size)


def _label_stats(x, labels, dev: bool, k: int):
    """-> host float64 (centroids [k, D], counts [k], sdist [k], within-cluster sum of squares, column means [D])."""
    n = int(x.shape[0])
    if dev:
        ops = cluster_ops
        zero_c = torch.zeros(k, int(x.shape[1]), dtype=torch.float64, device=x.device)
        cent, _, _ = ops.km_update(x, labels, torch.zeros(n, dtype=torch.float64, device=x.device), zero_c)
        wss, sdist, counts = ops.km_scores(labels, ops.km_label_dist(x, cent, labels), k)
        return (cent.cpu().numpy(), counts.cpu().numpy().astype(np.float64), sdist.cpu().numpy(), float(wss.item()),
                ops.km_colstats(x)[0].cpu().numpy())
    cent, counts, _, _, _ = update_host(x, labels, np.zeros(n), np.zeros((k, x.shape[1])))
    s = sqdist_host(x, cent)[np.arange(n), labels] if n * k <= (1 << 24) else np.concatenate(
        [sqdist_host(x[a:b], cent)[np.arange(b - a), labels[a:b]] for a, b in neighbors._host_blocks(n, k)])
    wss, sdist, _ = scores_host(labels, s, k)
    return cent, counts.astype(np.float64), sdist, wss, x.astype(np.float64).mean(axis=0)


def _db(cent, counts, sdist) -> float:
    intra = sdist / counts
    cd = np.sqrt(((cent[:, None, :] - cent[None, :, :]) ** 2).sum(axis=2))
    if np.allclose(intra, 0) or np.allclose(cd, 0):
        return 0.0
    cd[cd == 0] = np.inf
    return float(np.mean(np.max((intra[:, None] + intra[None, :]) / cd, axis=1)))


def _ch(cent, counts, wss, mean, n) -> float:
    k = cent.shape[0]
    extra = float((counts * ((cent - mean[None, :]) ** 2).sum(axis=1)).sum())
    return 1.0 if wss == 0.0 else extra * (n - k) / (wss * (k - 1.0))


def _scored(x, labels, what: str):
    x, dev = _rows(x, "x")
    n = int(x.shape[0])
    labels, k = _compact(labels, n, dev, x.device if dev else None)
    if not 2 <= k <= min(n - 1, MAX_K):
        raise ValueError(f"{what}: {k} distinct labels; valid values are 2 to min(n - 1, {MAX_K}) = {min(n - 1, MAX_K)}")
    return x, dev, n, labels, k


def davies_bouldin(x, labels) -> float:
    """``sklearn.metrics.davies_bouldin_score(x, labels)``: centroids = the label means, from the fixed-order sums."""
    x, dev, n, labels, k = _scored(x, labels, "davies_bouldin")
    cent, counts, sdist, _, _ = _label_stats(x, labels, dev, k)
    return _db(cent, counts, sdist)


def calinski_harabasz(x, labels) -> float:
    """``sklearn.metrics.calinski_harabasz_score(x, labels)``."""
    x, dev, n, labels, k = _scored(x, labels, "calinski_harabasz")
    cent, counts, _, wss, mean = _label_stats(x, labels, dev, k)
    return _ch(cent, counts, wss, mean, n)


def _queries(queries, n: int, dev: bool, device):
    if queries is None:
        return None
    q = _host(queries).reshape(-1).astype(np.int64)
    if q.size < 1 or q.min() < 0 or q.max() >= n:
        raise ValueError(f"silhouette_samples: queries must be row ids in [0, {n})")
    return torch.from_numpy(q.astype(np.int32)).to(device) if dev else q


def _silhouette(x, dev, n, labels, k, queries, want_mean=False):
    q = _queries(queries, n, dev, x.device if dev else None)
    if dev:
        counts = torch.bincount(labels.long(), minlength=k).to(torch.int32)
        sil, mean = cluster_ops.km_silhouette(x, labels, counts, q, want_mean)
        return sil, (float(mean.item()) if want_mean else None)
    sil = silhouette_samples_host(x, labels, q)
    return sil, (float(sil.mean()) if want_mean else None)


def silhouette_samples(x, labels, queries=None):
    """``sklearn.metrics.silhouette_samples(x, labels)`` (Euclidean) -> fp64 [n], or with ``queries`` (row ids) the
    coefficients of those rows alone, each still taken against ALL rows -> fp64 [len(queries)]."""
    x, dev, n, labels, k = _scored(x, labels, "silhouette_samples")
    return _silhouette(x, dev, n, labels, k, queries)[0]


def silhouette_score(x, labels, sample_size: Optional[int] = None, seed: int = 0) -> float:
    """The mean silhouette coefficient.  ``sample_size``: the mean over that many rows drawn without replacement by
    ``numpy.random.RandomState(seed)`` -- unlike sklearn's ``sample_size``, which scores the sample against itself, every
    drawn row is scored against ALL rows, so the sampled score estimates the full one."""
    x, dev, n, labels, k = _scored(x, labels, "silhouette_score")
    q = None
    if sample_size is not None and int(sample_size) < n:
        if int(sample_size) < 1:
            raise ValueError(f"silhouette_score: sample_size = {sample_size} must be at least 1")
        q = np.sort(np.random.RandomState(seed).choice(n, int(sample_size), replace=False))
    return _silhouette(x, dev, n, labels, k, q, True)[1]


def cluster_scores(x, result, sample_size: Optional[int] = None, seed: int = 0) -> dict:
    """``{"inertia", "davies_bouldin", "calinski_harabasz", "silhouette", "smallest_cluster"}`` of a ``KMeansResult`` (or
    of plain labels, then without the inertia) over the rows ``x``; ``sample_size`` as for ``silhouette_score``."""
    labels = result.labels if isinstance(result, KMeansResult) else result
    x, dev, n, lab, k = _scored(x, labels, "cluster_scores")
    cent, counts, sdist, wss, mean = _label_stats(x, lab, dev, k)
    q = None
    if sample_size is not None and int(sample_size) < n:
        q = np.sort(np.random.RandomState(seed).choice(n, int(sample_size), replace=False))
    return {"inertia": float(result.inertia) if isinstance(result, KMeansResult) else float(wss),
            "davies_bouldin": _db(cent, counts, sdist), "calinski_harabasz": _ch(cent, counts, wss, mean, n),
            "silhouette": _silhouette(x, dev, n, lab, k, q, True)[1], "smallest_cluster": int(counts.min())}


def k_sweep(x, ks: Sequence[int], init="k-means++", n_init: int = 1, max_iter: int = 300, tol: float = 1e-4, seed: int = 0,
            sample_size: Optional[int] = None) -> pd.DataFrame:
    """``kmeans`` and ``cluster_scores`` for every k of ``ks`` (each at least 2) -> frame (k, inertia, davies_bouldin,
    calinski_harabasz, silhouette, n_iter, smallest_cluster)."""
    rows = []
    for k in ks:
        res = kmeans(x, int(k), init=init, n_init=n_init, max_iter=max_iter, tol=tol, seed=seed)
        rows.append({"k": int(k), "n_iter": res.n_iter, **cluster_scores(x, res, sample_size, seed)})
    return pd.DataFrame(rows, columns=SWEEP_COLUMNS)


# ---------------------------------------------------------------------------- over a model's embeddings
def _ids(graph, node_type: str, n: int):
    ix = neighbors._indexer(graph, node_type)
    return [ix["index_to_id"][i] for i in range(n)] if ix is not None else np.arange(n, dtype=np.int64)


def patient_clusters(model, graph, n_clusters: int = 8, space: str = "final", seed: int = 42, output_dir=None,
                     lab_names=None, n_init: int = 1, max_iter: int = 300, sample_size: Optional[int] = 16384) -> dict:
    """K-means cohorts of ALL patients of the graph in the model's embedding space (``init="k-means++"``).
    -> {"result": KMeansResult, "patients": frame (patient_id -- through ``graph.indexers["patient"]`` when the graph has
    one --, cluster, distance to the cluster's centre), "summary": frame (cluster, n_patients, mean_lab_degree,
    median_lab_degree, mean_distance, silhouette_mean -- over ``sample_size`` sampled patients, each scored against all),
    "lab_profile": frame per cluster x lab with an observation (cluster, lab_idx, lab_name, n_observed = has_lab edges of
    the cluster's patients to the lab, coverage = n_observed / n_patients, mean_value and std_value (population) of the
    edges' normalised values)}.  With ``output_dir``: ``patient_clusters.csv``, ``cluster_summary.csv``,
    ``cluster_lab_profile.csv``."""
    from . import ops
    x = neighbors._node_embeddings(model, graph, space, "patient_clusters")["patient"]
    n, k = int(x.shape[0]), _check_k(n_clusters, int(x.shape[0]), "patient_clusters", 2)
    res = kmeans(x, k, n_init=n_init, max_iter=max_iter, seed=seed)
    labels = res.labels.long()
    dist = res.sqdist.sqrt()
    patients = pd.DataFrame({"patient_id": _ids(graph, "patient", n), "cluster": labels.cpu().numpy(),
                             "distance": dist.cpu().numpy()}, columns=PATIENT_CLUSTER_COLUMNS)
    # the silhouette of a seeded sample, averaged per cluster
    q = np.arange(n) if sample_size is None or int(sample_size) >= n else \
        np.sort(np.random.RandomState(seed).choice(n, int(sample_size), replace=False))
    counts = res.counts.cpu().numpy().astype(np.int64)
    sil_mean = np.full(k, np.nan)
    if int((counts > 0).sum()) >= 2:
        sil = silhouette_samples(x, res.labels, q)
        sil, ql = sil.cpu().numpy(), labels.cpu().numpy()[q]
        for c in range(k):
            if (ql == c).any():
                sil_mean[c] = float(sil[ql == c].mean())
    graph_dev = graph.to(x.device)
    ei = graph_dev[LAB_EDGE].edge_index
    pat, lab = ei[0].contiguous(), ei[1].contiguous()
    val = graph_dev[LAB_EDGE].edge_attr.reshape(-1).float().contiguous()
    deg = torch.bincount(pat, minlength=n).cpu().numpy()
    lab_host = labels.cpu().numpy()
    sdist = res.sdist.cpu().numpy()
    summary = pd.DataFrame({
        "cluster": np.arange(k), "n_patients": counts,
        "mean_lab_degree": [float(deg[lab_host == c].mean()) if counts[c] else np.nan for c in range(k)],
        "median_lab_degree": [float(np.median(deg[lab_host == c])) if counts[c] else np.nan for c in range(k)],
        "mean_distance": [float(sdist[c] / counts[c]) if counts[c] else np.nan for c in range(k)],
        "silhouette_mean": sil_mean}, columns=CLUSTER_SUMMARY_COLUMNS)
    n_labs = int(graph["lab"].num_nodes)
    given = embed._names_of(graph, "lab", lab_names)
    edge_cluster = labels[pat]
    zero = torch.zeros_like(val)
    none = torch.full_like(lab, -1)
    frames = []
    for c in range(k):
        # one segment reduction per cluster: segment = the lab where the patient is in the cluster, -1 elsewhere
        sums = ops.seg_sums(zero, val, torch.where(edge_cluster == c, lab, none).contiguous(), n_labs)[0].cpu().numpy()
        cnt, st, st2 = sums[:, 0], sums[:, 3], sums[:, 4]
        seen = np.flatnonzero(cnt > 0)
        mean = st[seen] / cnt[seen]
        frames.append(pd.DataFrame({
            "cluster": c, "lab_idx": seen, "lab_name": [given.get(int(i), f"lab_{int(i)}") for i in seen],
            "n_observed": cnt[seen].astype(np.int64), "coverage": cnt[seen] / max(int(counts[c]), 1), "mean_value": mean,
            "std_value": np.sqrt(np.maximum(st2[seen] / cnt[seen] - mean * mean, 0.0))}, columns=LAB_PROFILE_COLUMNS))
    profile = pd.concat(frames, ignore_index=True) if frames else pd.DataFrame(columns=LAB_PROFILE_COLUMNS)
    out = {"result": res, "patients": patients, "summary": summary, "lab_profile": profile}
    if output_dir is not None:
        d = Path(output_dir)
        d.mkdir(parents=True, exist_ok=True)
        patients.to_csv(d / "patient_clusters.csv", index=False)
        summary.to_csv(d / "cluster_summary.csv", index=False)
        profile.to_csv(d / "cluster_lab_profile.csv", index=False)
        logging.info(f"  Saved patient clusters to {d}")
    return out


def lab_clusters(model, graph, n_clusters: int, space: str = "initial", seed: int = 42, output_dir=None, lab_names=None,
                 n_init: int = 1, max_iter: int = 300) -> dict:
    """K-means clusters of the lab embeddings with the ``embed.lab_panels`` panel of every lab -- the table behind "labs
    cluster by clinical function".  -> {"result": KMeansResult, "labs": frame (lab_idx, lab_name, panel, cluster,
    distance), "panel_table": frame cluster x panel of lab counts}.  With ``output_dir``: ``lab_clusters.csv`` and
    ``lab_cluster_panel_table.csv``."""
    x = neighbors._node_embeddings(model, graph, space, "lab_clusters")["lab"]
    n, k = int(x.shape[0]), _check_k(n_clusters, int(x.shape[0]), "lab_clusters")
    res = kmeans(x, k, n_init=n_init, max_iter=max_iter, seed=seed)
    given = embed._names_of(graph, "lab", lab_names)
    names = {i: given.get(i, f"lab_{i}") for i in range(n)}
    panels = embed.lab_panels(names)
    labs = pd.DataFrame({"lab_idx": np.arange(n, dtype=np.int64), "lab_name": [names[i] for i in range(n)],
                         "panel": [panels[i] for i in range(n)], "cluster": _host(res.labels).astype(np.int64),
                         "distance": np.sqrt(_host(res.sqdist))}, columns=LAB_CLUSTER_COLUMNS)
    table = pd.crosstab(labs["cluster"], labs["panel"]).reindex(range(k), fill_value=0)
    table.index.name = "cluster"
    out = {"result": res, "labs": labs, "panel_table": table}
    if output_dir is not None:
        d = Path(output_dir)
        d.mkdir(parents=True, exist_ok=True)
        labs.to_csv(d / "lab_clusters.csv", index=False)
        table.to_csv(d / "lab_cluster_panel_table.csv")
        logging.info(f"  Saved lab clusters to {d}")
    return out
