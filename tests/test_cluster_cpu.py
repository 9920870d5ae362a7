"""mmgnn.cluster without a GPU: the float64 host path against sklearn (KMeans(init=array, n_init=1, algorithm="lloyd") and
the three cluster scores on float64 inputs), against the independent restatement tests/cluster_ref.py (equal, including
two clusters empty at once, which sklearn leaves to the order of an argpartition), the tie rules on a lattice, the
refusals, and the header's symbols through the binding.

Allowances against sklearn.  Labels and n_iter must be equal; the test first asserts that the smallest relative gap
between a row's best and second-best key over the whole run exceeds 1e-9 (measured here: 3.6e-5 or more), so that a
different summation order cannot move a row.  For centres, inertia and scores the distance between the host path and
sklearn was measured on these cases (it is printed by the tests) and the assertion allows 64 x the largest measured
value; the margin is for sklearn's summation order, which differs between BLAS builds:
  centres 1.1e-14 absolute, inertia 6e-16 relative, silhouette 4.4e-15, Davies-Bouldin 5.6e-15, Calinski-Harabasz
  1.2e-15 relative."""
import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import cluster, cluster_ops
import cluster_ref as cr

MIN_GAP = 1e-9
MARGIN = 64.0
CENTER_ABS, INERTIA_REL, SIL_ABS, DB_ABS, CH_REL = 1.1e-14, 6e-16, 4.4e-15, 5.6e-15, 1.2e-15
SHAPES = [(65, 3, 2), (500, 16, 8), (3000, 2, 5), (1000, 32, 64), (2000, 128, 16)]


def _case(n, D, k):
    x = cr.blobs(n, D, k, seed=n)
    return x, cr.init_rows(x, k)


def _empty_case(n_far):
    """k = 5 (or 6) centres of which n_far lie at 1e3, 2e3: empty in iteration 1."""
    x = cr.blobs(400, 8, 4, seed=7)
    init = x[:4 + n_far].astype(np.float64).copy()
    for e in range(n_far):
        init[2 + e] = 1e3 * (e + 1)
    return x, init


def _sklearn_kmeans(x, init):
    from sklearn.cluster import KMeans
    return KMeans(init.shape[0], init=init, n_init=1, algorithm="lloyd").fit(x.astype(np.float64))


def _against_sklearn(x, init):
    res = cluster.kmeans(x, init.shape[0], init=init)
    assert res.min_gap > MIN_GAP, res.min_gap
    km = _sklearn_kmeans(x, init)
    d_cent = float(np.abs(res.cluster_centers - km.cluster_centers_).max())
    d_inertia = abs(res.inertia - km.inertia_) / km.inertia_
    print(f"kmeans {x.shape} k={init.shape[0]}: gap {res.min_gap:.3g} centres {d_cent:.3g} inertia {d_inertia:.3g}")
    assert np.array_equal(res.labels, km.labels_)
    assert res.n_iter == km.n_iter_
    assert res.converged
    assert d_cent <= MARGIN * CENTER_ABS
    assert d_inertia <= MARGIN * INERTIA_REL
    assert np.array_equal(res.counts, np.bincount(km.labels_, minlength=init.shape[0]))
    return res, km


@pytest.mark.parametrize("n,D,k", SHAPES)
def test_host_kmeans_matches_sklearn(n, D, k):
    _against_sklearn(*_case(n, D, k))


def test_host_kmeans_matches_sklearn_with_one_empty_cluster():
    x, init = _empty_case(1)
    lab, min_s, _ = cluster.assign_host(x, init)
    _, _, _, m, rows = cluster.update_host(x, lab, min_s, init)
    assert m == 1 and rows.tolist() == [int(np.argmax(min_s))]
    _against_sklearn(x, init)


@pytest.mark.parametrize("case", ["blobs", "one_empty", "two_empty"])
def test_host_kmeans_equals_reference(case):
    if case == "blobs":
        x, init = _case(500, 16, 8)
    else:
        x, init = _empty_case(1 if case == "one_empty" else 2)
    if case == "two_empty":
        lab, min_s = cr.assign(x, init)
        new, counts, _, m, rows = cr.update(x, lab, min_s, init)
        assert m == 2 and counts[2] == 1 and counts[3] == 1
        order = np.argsort(-min_s, kind="stable")
        assert rows.tolist() == order[:2].tolist()           # cluster 2 takes the farthest row, cluster 3 the next
        assert np.array_equal(new[2], x[rows[0]].astype(np.float64)) and np.array_equal(new[3], x[rows[1]].astype(np.float64))
        h = cluster.update_host(x, lab, min_s, init)
        assert np.array_equal(h[0], new) and np.array_equal(h[1], counts) and h[2:4] == (cr.update(x, lab, min_s, init)[2], 2)
        assert np.array_equal(h[4], rows)
    res = cluster.kmeans(x, init.shape[0], init=init)
    centers, labels, inertia, n_iter, counts, min_s = cr.kmeans(x, init)
    assert np.array_equal(res.labels, labels) and res.n_iter == n_iter
    assert np.array_equal(res.cluster_centers, centers)
    assert res.inertia == inertia
    assert np.array_equal(res.counts, counts) and np.array_equal(res.sqdist, min_s)


@pytest.mark.parametrize("n,D,k", [(65, 3, 2), (500, 16, 8), (300, 5, 64)])
def test_host_scores_match_sklearn(n, D, k):
    from sklearn.metrics import calinski_harabasz_score, davies_bouldin_score, silhouette_samples
    x, init = _case(n, D, k)
    labels = cluster.kmeans(x, k, init=init).labels
    x64 = x.astype(np.float64)
    d_sil = float(np.abs(cluster.silhouette_samples(x, labels) - silhouette_samples(x64, labels)).max())
    d_db = abs(cluster.davies_bouldin(x, labels) - davies_bouldin_score(x64, labels))
    ch = calinski_harabasz_score(x64, labels)
    d_ch = abs(cluster.calinski_harabasz(x, labels) - ch) / ch
    print(f"scores {x.shape} k={k}: silhouette {d_sil:.3g} davies_bouldin {d_db:.3g} calinski_harabasz {d_ch:.3g}")
    assert d_sil <= MARGIN * SIL_ABS and d_db <= MARGIN * DB_ABS and d_ch <= MARGIN * CH_REL
    assert np.allclose(cluster.silhouette_samples(x, labels), cr.silhouette(x, labels), rtol=0, atol=MARGIN * SIL_ABS)
    q = np.array([3, 0, n - 1])
    assert np.array_equal(cluster.silhouette_samples(x, labels, queries=q), cluster.silhouette_samples(x, labels)[q])
    scores = cluster.cluster_scores(x, labels)
    assert abs(scores["silhouette"] - float(silhouette_samples(x64, labels).mean())) <= MARGIN * SIL_ABS
    assert scores["smallest_cluster"] == int(np.bincount(labels).min())


def test_silhouette_of_a_singleton_cluster_is_zero():
    x = np.array([[0, 0], [0, 1], [1, 0], [9, 9], [5, 5], [5, 6]], np.float32)
    labels = np.array([0, 0, 0, 1, 2, 2])
    s = cluster.silhouette_samples(x, labels)
    assert s[3] == 0.0 and np.all(s[[0, 1, 2, 4, 5]] > 0)
    assert np.array_equal(s, cr.silhouette(x, labels))


def test_ties_go_to_the_smaller_centre_and_the_smaller_row():
    # rows on the integer line between centres at -2, 2 and a copy of the centre at 2: x = 0 is equidistant
    x = np.array([[-3], [0], [0], [3], [1], [-1]], np.float32)
    centers = np.array([[-2.0], [2.0], [2.0]])
    labels, min_s = cluster.assign(x, centers)
    assert labels.tolist() == [0, 0, 0, 1, 1, 0] and min_s.tolist() == [1.0, 4.0, 4.0, 1.0, 1.0, 1.0]
    # cluster 2 is empty: it takes the row with the largest min_s, of the two at 4.0 the smaller row (1), not row 2
    new, counts, shift, m, rows = cluster.update_host(x, labels, min_s, centers)
    assert m == 1 and rows.tolist() == [1] and counts.tolist() == [3, 2, 1]
    assert new.tolist() == [[(-3 + 0 - 1) / 3.0], [2.0], [0.0]]
    ref = cr.update(x, labels, min_s, centers)
    assert np.array_equal(ref[0], new) and ref[4].tolist() == [1]
    # a lattice: every sum exact, the host path and the reference agree on every tie
    xl, cl = cr.lattice(300, 4, 3), cr.lattice(9, 4, 4).astype(np.float64)
    la, sa = cluster.assign(xl, cl)
    lb, sb = cr.assign(xl, cl)
    assert np.array_equal(la, lb) and np.array_equal(sa, sb)
    assert (np.sort(cr.sqdist(xl, cl), axis=1)[:, 0] == np.sort(cr.sqdist(xl, cl), axis=1)[:, 1]).any(), "no real tie"


def test_a_cluster_left_without_rows_keeps_its_centre():
    # cluster 1 holds row 2 alone and loses it to the empty cluster 2
    x = np.array([[0], [1], [10]], np.float32)
    labels, min_s = np.array([0, 0, 1], np.int32), np.array([0.25, 0.25, 4.0])
    new, counts, _, m, rows = cluster.update_host(x, labels, min_s, np.array([[0.5], [8.0], [50.0]]))
    assert m == 1 and rows.tolist() == [2] and counts.tolist() == [2, 0, 1]
    assert new.tolist() == [[0.5], [8.0], [10.0]]


def test_kmeans_plusplus_is_seeded_and_n_init_keeps_the_best():
    x = cr.blobs(600, 6, 5, seed=3)
    a, b = cluster.kmeans_plusplus(x, 5, seed=4), cluster.kmeans_plusplus(x, 5, seed=4)
    assert np.array_equal(a, b) and a.shape == (5, 6) and a.dtype == np.float64
    assert all((x.astype(np.float64) == c).all(axis=1).any() for c in a), "a centre that is no row of x"
    runs = [cluster.kmeans(x, 5, seed=s) for s in (0, 1, 2)]
    best = cluster.kmeans(x, 5, n_init=3, seed=0)
    assert best.inertia == min(r.inertia for r in runs)
    first = next(r for r in runs if r.inertia == best.inertia)
    assert np.array_equal(best.labels, first.labels)
    frame = cluster.k_sweep(x, [2, 5], seed=0)
    assert list(frame.columns) == cluster.SWEEP_COLUMNS and frame["k"].tolist() == [2, 5]
    assert frame["inertia"][0] > frame["inertia"][1]


def test_refusals():
    x = cr.blobs(40, 3, 2, seed=0)
    with pytest.raises(ValueError, match=r"D = 257 outside \[1, 256\]"):
        cluster.kmeans(np.zeros((300, 257), np.float32), 2)
    with pytest.raises(ValueError, match=r"n_clusters = 129 outside \[1, 128\]"):
        cluster.kmeans(cr.blobs(200, 3, 2, seed=0), 129)
    with pytest.raises(ValueError, match="n_clusters = 0 outside"):
        cluster.kmeans(x, 0)
    with pytest.raises(ValueError, match="exceeds the 40 rows"):
        cluster.kmeans(x, 41)
    with pytest.raises(TypeError, match="floating-point"):
        cluster.kmeans(np.zeros((40, 3), np.int64), 2)
    with pytest.raises(ValueError, match="expected \\[n, D\\] rows, got 1 dimensions"):
        cluster.kmeans(np.zeros(40, np.float32), 2)
    with pytest.raises(ValueError, match=r"init has shape \(3, 3\), expected \(2, 3\)"):
        cluster.kmeans(x, 2, init=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="k-means\\+\\+"):
        cluster.kmeans(x, 2, init="random")
    with pytest.raises(ValueError, match="n_init must be 1"):
        cluster.kmeans(x, 2, init=np.zeros((2, 3)), n_init=2)
    with pytest.raises(ValueError, match="centers has shape"):
        cluster.assign(x, np.zeros((2, 4)))
    with pytest.raises(ValueError, match="distinct labels"):
        cluster.silhouette_samples(x, np.zeros(40, np.int64))
    with pytest.raises(ValueError, match="row ids in"):
        cluster.silhouette_samples(x, np.arange(40) % 2, queries=[40])
    with pytest.raises(ValueError, match="labels has 39 entries"):
        cluster.davies_bouldin(x, np.zeros(39, np.int64))

    class Sharded(torch.nn.Module):
        _comm = object()
    for fn in (cluster.patient_clusters, cluster.lab_clusters):
        with pytest.raises(NotImplementedError, match="patient-sharded model"):
            fn(Sharded(), None, 2)


def test_binding_is_derived_from_the_header_without_loading_the_library():
    assert (cluster_ops.KM_MAX_K, cluster_ops.KM_MAX_D, cluster_ops.KM_ROW_TILE) == (128, 256, 64)
    assert (cluster_ops.KM_MAX_RANGES, cluster_ops.KM_MAX_GRID) == (128, 1024)
    assert (cluster.MAX_K, cluster.MAX_D) == (128, 256)
    calls = {"mmg_km_assign", "mmg_km_update", "mmg_km_colstats", "mmg_km_scores", "mmg_km_silhouette", "mmg_km_label_dist"}
    assert calls | {"mmg_km_plan", "mmg_km_sil_plan"} <= set(cluster_ops.SIGNATURES)
    for name in calls - {"mmg_km_label_dist"}:
        assert name + "_ws_bytes" in cluster_ops.SIGNATURES, name
        assert [p[0] for p in cluster_ops.PARAMS[name]][-3:] == ["ws", "ws_bytes", "stream"], name
    assert [p[0] for p in cluster_ops.PARAMS["mmg_km_assign"]][:7] == ["X", "n", "D", "ld_x", "C", "k", "prev_labels"]
