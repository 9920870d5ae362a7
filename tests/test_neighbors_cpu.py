"""Neighbours and map quality without a GPU (mmgnn/neighbors.py): the float64 host path -- the checker of
test_neighbors_gpu.py -- against sklearn's NearestNeighbors(algorithm="brute") and manifold.trustworthiness and against
the independent restatement tests/nn_ref.py, the tie rule, the refusals and the C symbols."""
import ctypes

import numpy as np
import pytest

import mmgnn  # noqa: F401
from mmgnn import _lib, neighbors as nb, nn_ops
import nn_ref as nr


@pytest.mark.parametrize("n, D", nr.GENERIC_SHAPES)
def test_host_search_equals_sklearn_brute_force(n, D):
    from sklearn.neighbors import NearestNeighbors
    x = nr.generic(n, D)
    gap = nr.min_relative_gap(x)
    print(f"({n}, {D}): smallest relative gap {gap:.3e}")
    assert gap > nr.MIN_GAP, "not a generic input: choose another seed"
    k = 10
    res = nb.nearest_neighbors(x, k)
    sk_d, sk_i = NearestNeighbors(n_neighbors=k, algorithm="brute").fit(x.astype(np.float64)).kneighbors()
    assert res.indices.dtype == np.int64 and res.distances.dtype == np.float32
    assert np.array_equal(res.indices, sk_i)
    assert np.abs(res.distances.astype(np.float64) - sk_d).max() <= 1e-5 * sk_d.max()     # sklearn takes the Gram form
    ri, rd = nr.knn(x, k)
    assert np.array_equal(res.indices, ri) and np.array_equal(res.distances, rd)
    # a separate query set: nothing skipped, a query that is a row finds it first at distance 0
    q = np.concatenate([x[:3], nr.generic(5, D, seed=9)])
    res = nb.nearest_neighbors(x, k, q)
    sk_i = NearestNeighbors(n_neighbors=k, algorithm="brute").fit(x.astype(np.float64)).kneighbors(q.astype(np.float64))[1]
    assert np.array_equal(res.indices, sk_i)
    assert np.array_equal(res.indices[:3, 0], [0, 1, 2]) and np.all(res.distances[:3, 0] == 0.0)


@pytest.mark.parametrize("n, D", nr.GENERIC_SHAPES)
def test_host_trustworthiness_equals_sklearn(n, D):
    from sklearn.manifold import trustworthiness
    x = nr.generic(n, D)
    y = nr.generic(n, 2, seed=3) + x[:, :2]                       # a map that keeps something of x
    assert min(nr.min_relative_gap(x), nr.min_relative_gap(y)) > nr.MIN_GAP
    for k in (5, 12):
        t = nb.trustworthiness(x, y, k)
        sk = trustworthiness(x.astype(np.float64), y.astype(np.float64), n_neighbors=k)
        c = nb.continuity(x, y, k)
        skc = trustworthiness(y.astype(np.float64), x.astype(np.float64), n_neighbors=k)
        print(f"({n}, {D}) k = {k}: trustworthiness {t!r} (sklearn differs by {t - sk:.1e}), continuity {c!r} ({c - skc:.1e})")
        assert abs(t - sk) <= 1e-12 and abs(c - skc) <= 1e-12
        assert t == nr.trustworthiness(x, y, k)
        q = nb.map_quality(x, y, k)
        assert q["trustworthiness"] == t and q["continuity"] == c
        a, b = nr.knn(x, k)[0], nr.knn(y, k)[0]
        want = np.mean([len(set(a[i]) & set(b[i])) / k for i in range(n)])
        assert abs(q["overlap"] - want) <= 1e-15 and q["overlap"] == nb.neighborhood_overlap(x, y, k)
    # t-SNE's float64 map is rounded once to fp32 first
    y64 = y.astype(np.float64) * (1.0 + 1e-12)
    assert nb.trustworthiness(x, y64, 5) == nb.trustworthiness(x, y64.astype(np.float32), 5)


def test_the_tie_rule_on_the_lattice_case():
    x = nr.lattice(200, 4, seed=5)
    k = 7
    order, s = nr.full_order(x)
    tied = int((s[:, k - 1] == s[:, k]).sum())
    dup = int((s[:, 0] == 0.0).sum())
    print(f"lattice [200, 4] k = {k}: {tied} rows tied at the k-th neighbour, {dup} rows duplicate another row")
    assert tied >= 100 and dup >= 10, "the lattice case has lost its ties"
    res = nb.nearest_neighbors(x, k)
    assert np.array_equal(res.indices, order[:, :k])
    assert np.array_equal(res.distances, np.sqrt(s[:, :k]).astype(np.float32))
    d2 = np.take_along_axis(nr.sums(x, x), res.indices, axis=1)
    assert np.all(np.diff(d2, axis=1) >= 0)
    same = np.diff(d2, axis=1) == 0
    assert same.any() and np.all(np.diff(res.indices, axis=1)[same] > 0), "equal sums are ordered by the smaller index"
    assert np.all(res.indices != np.arange(200)[:, None])
    # ranks: the inverse of the full order; invalid entries give 0
    nbr = np.random.default_rng(1).integers(0, 200, size=(200, 9))
    nbr[:, 0] = -1
    nbr[:, 1] = 200
    nbr[:, 2] = np.arange(200)
    r = nb.neighbor_ranks(x, nbr)
    assert r.dtype == np.int32 and np.array_equal(r, nr.ranks(x, nbr))
    assert np.all(r[:, :3] == 0)
    valid = nbr[:, 3:] != np.arange(200)[:, None]
    assert np.all(r[:, 3:][valid] >= 1) and np.all(r[:, 3:][~valid] == 0)
    rr = nb.neighbor_ranks(x, res.indices)
    assert np.array_equal(rr, np.broadcast_to(np.arange(1, k + 1), rr.shape))
    # all rows equal: the k smallest indices
    ones = np.ones((9, 3), np.float32)
    res = nb.nearest_neighbors(ones, 4)
    assert np.array_equal(res.indices, [[j for j in range(9) if j != i][:4] for i in range(9)]) and np.all(res.distances == 0)
    # a non-finite sum orders as +inf, among themselves by index
    bad = nr.generic(12, 3)
    bad[4, 1] = np.nan
    bad[7, 0] = np.inf
    res = nb.nearest_neighbors(bad, 11)
    assert np.array_equal(res.indices[0, -2:], [4, 7]) and np.all(np.isinf(res.distances[0, -2:]))
    assert np.array_equal(res.indices, nr.knn(bad, 11)[0])


def test_refusals():
    x = nr.generic(20, 4)
    for k in (0, 20, 129):
        with pytest.raises(ValueError, match="k = "):
            nb.nearest_neighbors(x, k)
    nb.nearest_neighbors(x, 19)
    nb.nearest_neighbors(x, 20, x[:2])                            # with queries k may be n
    with pytest.raises(ValueError, match="k = 21"):
        nb.nearest_neighbors(x, 21, x[:2])
    with pytest.raises(ValueError, match="k = 129"):
        nb.nearest_neighbors(nr.generic(300, 2), 129)
    with pytest.raises(ValueError, match="D = 257"):
        nb.nearest_neighbors(nr.generic(10, 257), 2)
    with pytest.raises(ValueError, match="columns"):
        nb.nearest_neighbors(x, 2, nr.generic(3, 5))
    with pytest.raises(ValueError, match="dimensions"):
        nb.nearest_neighbors(x[0], 2)
    with pytest.raises(TypeError, match="floating"):
        nb.nearest_neighbors(np.zeros((5, 2), np.int64), 2)
    y = nr.generic(20, 2)
    for fn in (nb.trustworthiness, nb.continuity, nb.neighborhood_overlap, nb.map_quality):
        with pytest.raises(ValueError, match="n_samples / 2"):
            fn(x, y, 10)                                          # n_neighbors >= n / 2, as sklearn refuses it
        with pytest.raises(ValueError, match="n_samples / 2"):
            fn(x, y, 0)
        fn(x, y, 9)
        with pytest.raises(ValueError, match="20 rows, y has 19"):
            fn(x, y[:19], 3)
    with pytest.raises(ValueError, match="neighbors has"):
        nb.neighbor_ranks(x, np.zeros((19, 3), np.int64))
    import torch

    class Sharded(torch.nn.Module):
        _comm = object()

    for fn in (nb.embedding_neighbors, nb.embedding_map_quality):
        with pytest.raises(NotImplementedError, match="sharded"):
            fn(Sharded(), None)
    with pytest.raises(NotImplementedError, match="sharded"):
        nb.similar_patients(Sharded(), None, [1])


def test_c_symbols_constants_and_host_side_refusals():
    ops = nn_ops                                                  # the binding derived from include/mmgnn_nn.h
    want = ["mmg_nn_search", "mmg_nn_search_ws_bytes", "mmg_nn_rank", "mmg_nn_rank_ws_bytes", "mmg_nn_plan"]
    assert sorted(want) == sorted(ops.SIGNATURES) == sorted(ops.PARAMS)
    assert not set(want) & set(_lib.SIGNATURES), "the training library's ABI is the one it had"
    lib = ops.load()
    for s in want:
        assert hasattr(lib, s)
    assert (ops.MMG_NN_MAX_K, ops.MMG_NN_QUERY_BLOCK, ops.MMG_NN_TILE) == (128, 64, 64)
    assert (ops.NN_MAX_K, ops.NN_QUERY_BLOCK, ops.NN_TILE, ops.NN_MAX_GRID) == (128, 64, 64, ops.MMG_NN_MAX_GRID)
    assert (nb.MAX_K, nb.MAX_D) == (ops.NN_MAX_K, ops.NN_MAX_D)
    assert ops.SIGNATURES["mmg_nn_search"][0] is ctypes.c_int and len(ops.SIGNATURES["mmg_nn_search"][1]) == 15
    assert [p[0] for p in ops.PARAMS["mmg_nn_rank"]] == ["X", "n", "D", "ld_x", "nbr", "ld_nbr", "k", "rank_out", "ld_rank",
                                                          "penalty_out", "ws", "ws_bytes", "stream"]
    # the size queries: 0 for an unsupported shape
    assert lib.mmg_nn_search_ws_bytes(100, 4, 100, 5) > 0 and lib.mmg_nn_rank_ws_bytes(100, 4, 5) > 0
    for args in ((0, 4, 1, 1), (100, 0, 100, 5), (100, 257, 100, 5), (100, 4, 0, 5), (100, 4, 100, 0), (100, 4, 100, 129),
                 (1 << 31, 4, 100, 5), (100, 4, 3, 101)):
        assert lib.mmg_nn_search_ws_bytes(*args) == 0, args
    for args in ((0, 4, 1), (100, 0, 5), (100, 257, 5), (100, 4, 0), (100, 4, 129), (1 << 31, 4, 5)):
        assert lib.mmg_nn_rank_ws_bytes(*args) == 0, args
    # the plan: ranges only with few query blocks, never an empty range, at most MAX_GRID workgroups
    B, G = ops.NN_QUERY_BLOCK, ops.NN_MAX_GRID
    assert ops.nn_plan(2) == (1, 1, 1) and ops.nn_plan(B + 1) == (1, 2, 2)
    ns, items, grid = ops.nn_plan(1000)
    assert ns == 4 and items == 16 * 4 and grid == items
    ns, items, grid = ops.nn_plan(1 << 20)
    assert ns == 1 and items == (1 << 20) // B and grid == G
    ns, items, grid = ops.nn_plan(1 << 20, 1)
    assert ns == 64 and items == 64 and grid == 64
    # every refusal is made on the host before anything is enqueued: no GPU is needed to see them
    x = (ctypes.c_float * 64)()
    out_d, out_i = (ctypes.c_float * 64)(), (ctypes.c_int64 * 64)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)                 # noqa: E731
    ws = (ctypes.c_uint8 * 4096)()

    def search(n, D, ld_x, q, nq, ld_q, k, ld_d, ld_i, nbytes=4096):
        rc = lib.mmg_nn_search(p(x), n, D, ld_x, q, nq, ld_q, k, p(out_d), ld_d, p(out_i), ld_i, p(ws), nbytes, None)
        return rc, _lib.load().mmg_last_error()

    def rank(n, D, ld_x, ld_nbr, k, ld_rank, nbytes=4096, with_rank=True):
        rc = lib.mmg_nn_rank(p(x), n, D, ld_x, p(out_i), ld_nbr, k, p(out_d) if with_rank else None, ld_rank, None,
                             p(ws), nbytes, None)
        return rc, _lib.load().mmg_last_error()

    E_ARG, E_WS = -1, -3
    for (rc, msg), word in ((search(0, 4, 4, None, 0, 0, 1, 1, 1), b"n 0"), (search(8, 0, 4, None, 8, 0, 1, 1, 1), b"D 0"),
                            (search(8, 257, 257, None, 8, 0, 1, 1, 1), b"D 257"), (search(8, 4, 3, None, 8, 0, 1, 1, 1), b"ld_x"),
                            (search(8, 4, 4, None, 7, 0, 1, 1, 1), b"self mode"), (search(8, 4, 4, p(x), 2, 3, 1, 1, 1), b"ld_q"),
                            (search(8, 4, 4, None, 8, 0, 0, 1, 1), b"k 0"), (search(8, 4, 4, None, 8, 0, 8, 8, 8), b"k 8"),
                            (search(8, 4, 4, p(x), 2, 4, 9, 9, 9), b"k 9"), (search(8, 4, 4, None, 8, 0, 3, 2, 3), b"ld_dist"),
                            (search(8, 4, 4, None, 8, 0, 3, 3, 2), b"ld_idx"), (rank(0, 4, 4, 1, 1, 1), b"n 0"),
                            (rank(8, 257, 257, 1, 1, 1), b"D 257"), (rank(8, 4, 3, 1, 1, 1), b"ld_x"),
                            (rank(8, 4, 4, 1, 129, 129), b"k 129"), (rank(8, 4, 4, 2, 3, 3), b"ld_nbr"),
                            (rank(8, 4, 4, 3, 3, 2), b"ld_rank"), (rank(8, 4, 4, 3, 3, 3, with_rank=False), b"neither")):
        assert rc == E_ARG and word in msg, (rc, msg, word)
    rc, msg = search(8, 4, 4, None, 8, 0, 3, 3, 3, nbytes=lib.mmg_nn_search_ws_bytes(8, 4, 8, 3) - 1)
    assert rc == E_WS and b"workspace" in msg
    rc, msg = rank(8, 4, 4, 3, 3, 3, nbytes=lib.mmg_nn_rank_ws_bytes(8, 4, 3) - 1)
    assert rc == E_WS and b"workspace" in msg
