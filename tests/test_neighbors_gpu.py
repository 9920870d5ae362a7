"""Nearest neighbours, ranks and map quality on the MI355X (csrc/nn.hip, mmgnn/neighbors.py) against the float64 host
restatement tests/nn_ref.py.  The result is defined by a total order, so on lattice inputs (small integers: every sum
exact, real ties) indices, distances and ranks must be EQUAL; on generic inputs the test first asserts the input's
smallest relative gap between consecutive sorted distances (nn_ref.MIN_GAP, far above the (D + 8) 2^-52 by which the
fma chain and the host's sums can differ), then asks for equal indices and ranks and distances within 1 fp32 ulp.

Shapes: B = ops.NN_QUERY_BLOCK = 64 query rows per workgroup, T = ops.NN_TILE = 64 candidates per LDS tile, K =
ops.NN_MAX_K = 128; n = 2, B - 1, B, B + 1 (= T - 1, T, T + 1) and 2 T + 3; BIG_N, taken from the library's own plan, is
the smallest n = m B + 1 at which the candidates are split into ranges (the merge kernel runs) AND there are more work
items than workgroups (a workgroup walks more than one); RANK_BIG_N = MAX_GRID * B + 1 makes a workgroup of the rank
kernel walk two query blocks.  Every buffer has a padded row stride whose sentinel padding must survive."""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import embed, neighbors as nb, nn_ops as ops
from mmgnn.model import build_model
from mmgnn.synth import make_graph
import nn_ref as nr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, T, K, G = ops.NN_QUERY_BLOCK, ops.NN_TILE, ops.NN_MAX_K, ops.NN_MAX_GRID
assert (B, T, K) == (64, 64, 128), "the shapes below are chosen for these switches"
SENTINEL = -12345.0
NS = sorted({2, B - 1, B + 1, T - 1, T, T + 1, 2 * T + 3})
DS = [1, 2, 3, 68, 128, 256]
BIG_N = next(n for n in range(B + 1, 1 << 17, B) if ops.nn_plan(n)[0] > 1 and ops.nn_plan(n)[1] > ops.nn_plan(n)[2])
RANK_BIG_N = G * B + 1


def _ks(n_candidates):
    return sorted({k for k in (1, 5, K, n_candidates) if 1 <= k <= min(K, n_candidates)})


def _make(kind, n, D, seed=0):
    """"lattice": integers -3 .. 3 (heavy ties); "wide": integers -2000 .. 2000 (exact sums, few ties); "generic"."""
    if kind == "generic":
        return nr.generic(n, D, seed)
    return nr.lattice(n, D, seed + 5, span=3 if kind == "lattice" else 2000)


def _big_rows(n):
    """The rows of a large case that are checked against the host: both ends, a random few, the rows around the first
    query block a re-used workgroup of the search takes, and those around the rank kernel's."""
    nsplit, _, grid = ops.nn_plan(n)
    rows = [np.arange(8), np.arange(n - 8, n), np.random.default_rng(2).integers(0, n, 24), (grid // nsplit) * B + np.arange(-2, 3)]
    if n > G * B:
        rows.append(np.arange(G * B - 2, n))
    rows = np.unique(np.concatenate(rows))
    return rows[(rows >= 0) & (rows < n)].astype(np.int64)


def _padded(a, pad=3, fill=1e6):
    """A host matrix -> a device buffer with `pad` more columns of a sentinel, and the view of the data in it."""
    buf = np.full((a.shape[0], a.shape[1] + pad), fill, a.dtype)
    buf[:, :a.shape[1]] = a
    t = torch.from_numpy(buf).to(DEV)
    return t, t[:, :a.shape[1]]


def _search(x, k, queries=None):
    """mmg_nn_search over padded inputs into padded outputs -> (indices, distances) on the host; the padding is checked."""
    xbuf, xd = _padded(x)
    qd = None if queries is None else _padded(queries, pad=5)[1]
    nq = x.shape[0] if queries is None else queries.shape[0]
    dbuf = torch.full((nq, k + 2), SENTINEL, device=DEV)
    ibuf = torch.full((nq, k + 3), -77, dtype=torch.int64, device=DEV)
    ops.nn_search(xd, k, qd, dist_out=dbuf[:, :k], idx_out=ibuf[:, :k])
    torch.cuda.synchronize()
    assert torch.all(dbuf[:, k:] == SENTINEL) and torch.all(ibuf[:, k:] == -77), "the padding of an output was written"
    assert torch.all(xbuf[:, x.shape[1]:] == 1e6)
    return ibuf[:, :k].cpu().numpy(), dbuf[:, :k].cpu().numpy()


def _check_search(kind, x, k, got_i, got_d, rows=None, queries=None, what=""):
    want_i, want_d = nr.knn(x, k, rows, queries)
    if rows is not None:
        got_i, got_d = got_i[rows], got_d[rows]
    assert np.array_equal(got_i, want_i), f"{what}: indices"
    if kind != "generic":                                          # exact sums: the same bits
        assert np.array_equal(got_d, want_d), f"{what}: distances"
    else:
        ulp = nr.ulp_diff(got_d, want_d).max()
        assert ulp <= 1.0, f"{what}: distances {ulp} ulp"


def _assert_generic(x, rows=None, queries=None):
    order, s = nr.full_order(x, rows, queries)
    d = np.sqrt(s)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = float(np.nanmin((d[:, 1:] - d[:, :-1]) / d[:, 1:])) if d.shape[1] > 1 else 1.0
    assert gap > nr.MIN_GAP, f"not a generic input (gap {gap:.3e}): choose another seed"
    return gap


@pytest.mark.parametrize("kind", ["lattice", "generic"])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("n", NS)
def test_search_self_mode(n, D, kind):
    x = _make(kind, n, D, seed=n + D)
    if kind == "generic":
        _assert_generic(x)
    for k in _ks(n - 1):
        got_i, got_d = _search(x, k)
        assert np.all(got_i != np.arange(n)[:, None]), "a row lists itself"
        _check_search(kind, x, k, got_i, got_d, what=f"n {n} D {D} k {k}")


@pytest.mark.parametrize("kind, D, k, seed", [("lattice", 3, 5, 1), ("lattice", 3, K, 1), ("generic", 16, 5, 1),
                                              ("generic", 128, K, 3)])
def test_search_where_a_workgroup_walks_several_items_and_the_ranges_are_merged(kind, D, k, seed):
    n = BIG_N
    nsplit, items, grid = ops.nn_plan(n)
    print(f"BIG_N = {n}: {nsplit} candidate ranges, {items} work items on {grid} workgroups")
    assert nsplit > 1 and items > grid
    x = _make(kind, n, D, seed=seed)
    rows = _big_rows(n)
    if kind == "generic":
        print(f"  gap {_assert_generic(x, rows):.3e}")
    got_i, got_d = _search(x, k)
    assert np.all(got_i != np.arange(n)[:, None])
    _check_search(kind, x, k, got_i, got_d, rows=rows, what=f"n {n} D {D} k {k}")
    # every row: in range, no index twice, ascending distances
    assert got_i.min() >= 0 and got_i.max() < n and np.all(np.diff(got_d, axis=1) >= 0)
    assert np.all(np.diff(np.sort(got_i, axis=1), axis=1) > 0)


@pytest.mark.parametrize("kind", ["lattice", "generic"])
@pytest.mark.parametrize("n, D, nq, k", [(B + 1, 3, 1, B + 1), (100, 68, B + 1, 100), (2 * T + 3, 2, B + 1, 5),
                                         (2 * T + 3, 256, 1, K), (1000, 16, 1, 5), (1000, 4, B + 1, K)])
def test_search_with_a_separate_query_set(n, D, nq, k, kind):
    x = _make(kind, n, D, seed=3)
    q = _make(kind, nq, D, seed=4)
    own = np.arange(nq) * 7 % n
    q[::2] = x[own[::2]]                                           # every other query IS a candidate row
    if kind == "generic":
        _assert_generic(x, queries=q)
    if n == 1000:
        assert ops.nn_plan(n, nq)[0] > 1, "this case is meant to split the candidates"
    got_i, got_d = _search(x, k, q)
    _check_search(kind, x, k, got_i, got_d, queries=q, what=f"n {n} D {D} nq {nq} k {k}")
    assert np.all(got_d[::2, 0] == 0.0), "a query that is a candidate row finds it at distance 0: nothing is skipped"
    if kind == "generic":
        assert np.array_equal(got_i[::2, 0], own[::2])
    if k == n:
        assert np.array_equal(np.sort(got_i, axis=1), np.broadcast_to(np.arange(n), (nq, n)))


def test_ties():
    # the lattice case of the issue
    x = nr.lattice(200, 4, seed=5)
    order, s = nr.full_order(x)
    assert int((s[:, 6] == s[:, 7]).sum()) >= 100
    got_i, got_d = _search(x, 7)
    assert np.array_equal(got_i, order[:, :7]) and np.array_equal(got_d, np.sqrt(s[:, :7]).astype(np.float32))
    # three equal rows among generic ones: each finds the other two first, the smaller index first
    x = nr.generic(150, 68, seed=8)
    x[90] = x[17]
    x[133] = x[17]
    got_i, got_d = _search(x, 5)
    assert got_i[17, :2].tolist() == [90, 133] and got_i[90, :2].tolist() == [17, 133] and got_i[133, :2].tolist() == [17, 90]
    assert np.all(got_d[[17, 90, 133], :2] == 0.0) and np.all(got_d[[17, 90, 133], 2] > 0.0)
    assert np.array_equal(got_i, nr.knn(x, 5)[0])
    # all rows equal: the k smallest indices -- one range, and ranges merged
    for n, D, k in ((150, 5, 4), (150, 5, K), (1000, 3, K)):
        x = np.full((n, D), 0.25, np.float32)
        got_i, got_d = _search(x, k)
        want = np.array([[j for j in range(k + 1) if j != i][:k] for i in range(n)])
        assert np.array_equal(got_i, want), (n, D, k)
        assert np.all(got_d == 0.0)
    # non-finite sums order as +inf, among themselves by index
    x = nr.generic(70, 3, seed=2)
    x[4, 1] = np.nan
    x[66, 0] = np.inf
    got_i, got_d = _search(x, 69)
    assert np.array_equal(got_i, nr.knn(x, 69)[0])
    assert got_i[0, -2:].tolist() == [4, 66] and np.all(np.isinf(got_d[0, -2:]))


def _rank_case(x, kk, seed=0):
    n = x.shape[0]
    nbr = np.random.default_rng(seed).integers(0, n, size=(n, kk)).astype(np.int64)
    if kk >= 3:
        nbr[:, 0] = -1
        nbr[:, 1] = n
        nbr[:, 2] = np.arange(n)
    return nbr


def _rank(x, nbr):
    """mmg_nn_rank with padded x, nbr and rank_out -> (ranks, penalty) on the host; and the penalty alone."""
    n, kk = nbr.shape
    xd = _padded(x)[1]
    nbuf, nd = _padded(nbr, pad=2, fill=5)                         # (a padding entry that would be a valid row)
    rbuf = torch.full((n, kk + 4), -9, dtype=torch.int32, device=DEV)
    rank, pen = ops.nn_rank(xd, nd, rank_out=rbuf[:, :kk])
    alone = ops.nn_rank(xd, nd, want_rank=False)
    torch.cuda.synchronize()
    assert alone[0] is None and int(alone[1].item()) == int(pen.item()), "the penalty alone differs"
    assert torch.all(rbuf[:, kk:] == -9) and torch.all(nbuf[:, kk:] == 5), "the padding was written"
    return rank.cpu().numpy(), int(pen.item())


@pytest.mark.parametrize("kind", ["lattice", "generic"])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("n", NS)
def test_rank_and_penalty(n, D, kind):
    x = _make(kind, n, D, seed=n + D)
    if kind == "generic":
        _assert_generic(x)
    for kk in (1, 5, K):
        nbr = _rank_case(x, kk, seed=kk)
        got, pen = _rank(x, nbr)
        want = nr.ranks(x, nbr)
        assert got.dtype == np.int32 and np.array_equal(got, want), f"n {n} D {D} k {kk}"
        assert pen == int(np.maximum(want.astype(np.int64) - kk, 0).sum())
        if kk >= 3:
            assert np.all(got[:, :3] == 0), "-1, n and i itself give rank 0"
    # the ranks of a row's own nearest neighbours are 1 .. k
    k = min(5, n - 1)
    idx = _search(x, k)[0]
    got, pen = _rank(x, idx)
    assert np.array_equal(got, np.broadcast_to(np.arange(1, k + 1), (n, k))) and pen == 0


@pytest.mark.parametrize("kind, n, D, kk", [("lattice", BIG_N, 3, 5), ("generic", BIG_N, 16, K), ("lattice", RANK_BIG_N, 2, 3),
                                            ("wide", RANK_BIG_N, 2, 3)])
def test_rank_at_the_large_sizes(kind, n, D, kk):
    """(a generic input of RANK_BIG_N rows in 2 columns cannot meet the gap precondition: the exact "wide" lattice
    stands in for it)"""
    x = _make(kind, n, D, seed=1)
    rows = _big_rows(n)
    if kind == "generic":
        print(f"  gap {_assert_generic(x, rows):.3e}")
    nbr = _rank_case(x, kk, seed=4)
    got, pen = _rank(x, nbr)
    assert np.array_equal(got[rows], nr.ranks(x, nbr, rows)), f"n {n} D {D} k {kk}"
    assert np.all(got[:, :3] == 0) and got.min() >= 0 and got.max() <= n - 1
    assert pen == int(np.maximum(got.astype(np.int64) - kk, 0).sum())


@pytest.mark.parametrize("n, D", [(300, 16), (257, 128), (1000, 128)])
def test_map_scores_equal_the_host_path_and_sklearn(n, D):
    from sklearn.manifold import trustworthiness
    x = nr.generic(n, D)
    y = nr.generic(n, 2, seed=3) + x[:, :2]
    assert min(nr.min_relative_gap(x), nr.min_relative_gap(y)) > nr.MIN_GAP
    xd, yd = _padded(x)[1], _padded(y)[1]
    for k in (5, 12):
        t, c, o = nb.trustworthiness(xd, yd, k), nb.continuity(xd, yd, k), nb.neighborhood_overlap(xd, yd, k)
        assert (t, c, o) == (nb.trustworthiness(x, y, k), nb.continuity(x, y, k), nb.neighborhood_overlap(x, y, k))
        sk_t = trustworthiness(x.astype(np.float64), y.astype(np.float64), n_neighbors=k)
        sk_c = trustworthiness(y.astype(np.float64), x.astype(np.float64), n_neighbors=k)
        print(f"({n}, {D}) k = {k}: trustworthiness {t!r} (sklearn {t - sk_t:+.1e}), continuity {c!r} ({c - sk_c:+.1e}), "
              f"overlap {o!r}")
        assert abs(t - sk_t) <= 1e-12 and abs(c - sk_c) <= 1e-12
        assert nb.map_quality(xd, yd, k) == {"trustworthiness": t, "continuity": c, "overlap": o}
    # the float64 map of t-SNE is rounded once to fp32 first
    y64 = torch.from_numpy(y.astype(np.float64) * (1.0 + 1e-12)).to(DEV)
    assert nb.trustworthiness(xd, y64, 5) == nb.trustworthiness(xd, y64.float(), 5)
    res = nb.nearest_neighbors(xd, 7)
    assert res.indices.is_cuda and res.indices.dtype == torch.int64 and res.distances.dtype == torch.float32
    r = nb.neighbor_ranks(xd, res.indices)
    assert r.is_cuda and r.dtype == torch.int32 and torch.all(r == torch.arange(1, 8, device=DEV, dtype=torch.int32))
    with pytest.raises(ValueError, match="n_samples / 2"):
        nb.trustworthiness(xd, yd, (n + 1) // 2)
    with pytest.raises(ValueError, match="k = "):
        nb.nearest_neighbors(xd, n)
    with pytest.raises(ValueError, match="both"):
        nb.trustworthiness(xd, y, 5)


@functools.lru_cache(maxsize=None)
def _model_and_graph():
    g = make_graph(1, seed=0).to(DEV)
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"}}
    torch.manual_seed(0)
    model = build_model(cfg, (g.node_types, g.edge_types), None).to(DEV)
    model._init_embeddings(g)
    model.train()
    return model, g


def _embeddings(model, g, space):
    model.eval()
    with torch.no_grad():
        x = model.encode_nodes(g) if space == "initial" else model(g)
    model.train()
    return {t: v.detach().float().cpu().numpy() for t, v in x.items()}


@pytest.mark.parametrize("space", ["final", "initial"])
def test_similar_patients(space):
    model, g = _model_and_graph()
    n = int(g["patient"].num_nodes)
    ids = [f"P{5 * i % n:05d}" for i in range(n)]                  # not the identity: index i has id ids[i]
    assert len(set(ids)) == n
    g.indexers = {"patient": {"id_to_index": {s: i for i, s in enumerate(ids)}, "index_to_id": dict(enumerate(ids))}}
    try:
        ask = [ids[3], ids[n - 1], ids[500], ids[3]]
        out = nb.similar_patients(model, g, ask, k=10, space=space)
    finally:
        del g._extra["indexers"]
    assert model.training
    assert list(out.columns) == nb.NEIGHBOR_COLUMNS and len(out) == len(ask) * 10
    assert out["patient_id"].tolist() == [a for a in ask for _ in range(10)]
    assert out["rank"].tolist() == list(range(1, 11)) * len(ask)
    x = _embeddings(model, g, space)["patient"]
    back = {s: i for i, s in enumerate(ids)}
    rows = np.array([back[a] for a in ask])
    print(f"patient embeddings ({space}): gap {_assert_generic(x, np.unique(np.concatenate([rows, [5, 9]]))):.3e}")
    want_i, want_d = nr.knn(x, 10, rows=rows)                     # over ALL patients, the patient itself left out
    got_i = np.array([back[s] for s in out["neighbor_id"]]).reshape(len(ask), 10)
    assert np.array_equal(got_i, want_i)
    assert nr.ulp_diff(out["distance"].to_numpy().reshape(len(ask), 10), want_d).max() <= 1.0
    # without indexers the ids are node indices
    out = nb.similar_patients(model, g, [5, 9], k=3, space=space)
    assert out["patient_id"].tolist() == [5, 5, 5, 9, 9, 9] and np.array_equal(
        out["neighbor_id"].to_numpy().reshape(2, 3), nr.knn(x, 3, rows=np.array([5, 9]))[0])
    with pytest.raises(KeyError):
        nb.similar_patients(model, g, [n], k=3)
    # the largest k: K - 1, since one of the K listed candidates is the patient itself
    out = nb.similar_patients(model, g, [5, n - 1], k=K - 1, space=space)
    rows = np.array([5, n - 1])
    _assert_generic(x, rows)
    assert np.array_equal(out["neighbor_id"].to_numpy().reshape(2, K - 1), nr.knn(x, K - 1, rows=rows)[0])
    with pytest.raises(ValueError, match=f"k = {K} outside \\[1, {K - 1}\\]"):
        nb.similar_patients(model, g, [5], k=K, space=space)


def test_embedding_neighbors_and_map_quality_leave_the_maps_alone(tmp_path):
    model, g = _model_and_graph()
    names = {i: s for i, s in enumerate(["pH", "PTT", "sodium", "potassium", "Hct", "Hgb", "ALT (SGPT)", "albumin"])}
    embed.embedding_maps(model, g, output_dir=tmp_path, lab_names=names)
    embed.embedding_tsne(model, g, max_points=300, seed=7, output_dir=tmp_path, lab_names=names)
    before = {f: open(tmp_path / f, "rb").read() for f in sorted(os.listdir(tmp_path))}
    assert len(before) == 11
    out = nb.embedding_neighbors(model, g, space="initial", k=5, output_dir=tmp_path, lab_names=names)
    n_labs = int(g["lab"].num_nodes)
    fr = pd.read_csv(tmp_path / "lab_neighbors.csv")
    assert list(fr.columns) == nb.LAB_NEIGHBOR_COLUMNS and len(fr) == n_labs * 5
    assert list(out["purity"].columns) == nb.PURITY_COLUMNS
    x = _embeddings(model, g, "initial")["lab"]
    print(f"lab embeddings: gap {_assert_generic(x):.3e}")
    want_i, want_d = nr.knn(x, 5)
    assert np.array_equal(fr["neighbor_idx"].to_numpy().reshape(n_labs, 5), want_i)
    assert nr.ulp_diff(out["neighbors"]["distance"].to_numpy().reshape(n_labs, 5), want_d).max() <= 1.0
    panels = embed.lab_panels({i: names.get(i, f"lab_{i}") for i in range(n_labs)})
    assert fr["panel"].tolist() == [panels[i] for i in fr["lab_idx"]]
    assert fr["neighbor_panel"].tolist() == [panels[j] for j in fr["neighbor_idx"]]
    assert fr["lab_name"][0] == "pH" and fr["neighbor_name"].tolist() == [names.get(j, f"lab_{j}") for j in fr["neighbor_idx"]]
    # the purity, recomputed on the host from the csv
    pu = pd.read_csv(tmp_path / "lab_panel_purity.csv").set_index("panel")
    same = fr["panel"] == fr["neighbor_panel"]
    assert pu.index[-1] == "all" and pu.loc["all", "n_neighbors"] == len(fr) and pu.loc["all", "same_panel"] == int(same.sum())
    assert abs(pu.loc["all", "purity"] - same.mean()) <= 1e-15
    for panel, grp in fr.groupby("panel"):
        m = grp["panel"] == grp["neighbor_panel"]
        assert pu.loc[panel, "n_labs"] == grp["lab_idx"].nunique() and abs(pu.loc[panel, "purity"] - m.mean()) <= 1e-15
    assert set(pu.index) == set(fr["panel"]) | {"all"} and {"ABG", "Coag", "CMP", "CBC", "LFT", "Other"} <= set(pu.index)

    q = nb.embedding_map_quality(model, g, space="initial", max_points=300, seed=7, output_dir=tmp_path)
    assert model.training
    assert list(q.columns) == nb.MAP_QUALITY_COLUMNS
    assert list(pd.read_csv(tmp_path / "map_quality.csv").columns) == nb.MAP_QUALITY_COLUMNS
    types = [t for t in ("lab", "diagnosis", "medication", "patient") if int(g[t].num_nodes) >= 4]
    assert q["node_type"].tolist() == [t for t in types for _ in range(2)] and q["method"].tolist() == ["pca", "tsne"] * len(types)
    pat = q[q["node_type"] == "patient"].set_index("method")
    assert pat.loc["pca", "n"] == 300 and pat.loc["pca", "n_neighbors"] == 5
    sc = q[["trustworthiness", "continuity", "overlap"]].to_numpy()
    assert np.all(np.isfinite(sc)) and np.all(sc >= 0.0) and np.all(sc <= 1.0)
    # the PCA row of the sampled patients, from the pieces
    pick = np.random.RandomState(7).choice(int(g["patient"].num_nodes), 300, replace=False)
    xp = torch.from_numpy(_embeddings(model, g, "initial")["patient"][pick]).to(DEV)
    assert nb.map_quality(xp, embed.pca(xp, 2).projection, 5) == {
        k: pat.loc["pca", k] for k in ("trustworthiness", "continuity", "overlap")}
    # nothing the existing calls wrote has changed
    after = {f: open(tmp_path / f, "rb").read() for f in before}
    assert after == before
    assert sorted(set(os.listdir(tmp_path)) - set(before)) == ["lab_neighbors.csv", "lab_panel_purity.csv", "map_quality.csv"]


def test_bitwise_reproducible_eager_and_replayed():
    n, D, k = 1000, 68, 10                                         # the candidates are split: both kernels of the search
    assert ops.nn_plan(n)[0] > 1
    x = torch.from_numpy(nr.lattice(n, D, seed=3) + nr.generic(n, D, seed=4) * np.float32(1e-3)).to(DEV)
    y = torch.from_numpy(nr.generic(n, 2, seed=5)).to(DEV)
    dist = torch.empty(n, k, device=DEV)
    idx = torch.empty(n, k, dtype=torch.int64, device=DEV)
    rank = torch.empty(n, k, dtype=torch.int32, device=DEV)
    pen = [None]

    def run():
        ops.nn_search(y, k, dist_out=dist, idx_out=idx)
        pen[0] = ops.nn_rank(x, idx, rank_out=rank)[1]

    def reset():
        dist.fill_(-1.0)
        idx.fill_(-1)
        rank.fill_(-1)

    def bits():
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (dist, idx, rank, pen[0])]

    reset()
    run()
    ref = bits()
    assert ref[3][0] > 0 and np.array_equal(ref[1], nr.knn(y.cpu().numpy(), k)[0])
    reset()
    run()
    for name, r, o in zip(("dist", "idx", "rank", "penalty"), ref, bits()):
        assert np.array_equal(r.view(np.uint8), o.view(np.uint8)), f"{name}: the second eager run differs"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                      # warm-up off the default stream, as torch.cuda.graph asks
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        reset()
        graph.replay()
        for name, r, o in zip(("dist", "idx", "rank", "penalty"), ref, bits()):
            assert np.array_equal(r.view(np.uint8), o.view(np.uint8)), f"{name}: a replayed capture differs from the eager run"
