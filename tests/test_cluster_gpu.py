"""K-means and the cluster scores on the MI355X (csrc/cluster.hip, mmgnn/cluster.py) against the float64 host path of
mmgnn.cluster (itself held to sklearn and to tests/cluster_ref.py by test_cluster_cpu.py).

Bounds, u = 2^-53.  The device and the host form the same differences x_id - C_cd (one rounding each, the same); the
device adds their squares with one fma per column, the host with a product and a sum, so for equal centres
  |min_s_dev - min_s_host| <= (D + 8) u min_s                                       (ASSIGN)
and on lattice inputs (small integers: every sum exact, real ties) labels and min_s are EQUAL.  For equal labels a centre
is a quotient of a sum of count_c exactly widened fp32 values taken in two different orders:
  |C_dev - C_host|[c][d] <= (count_c + 8) u sum_{i in c} |x_id| / count_c            (UPDATE)
The shift sum_cd (new - old)^2 inherits 2 |new - old| e + e^2 per term from a centre error e, plus (k D + 8) u shift for
its own sums.  A whole run repeats this: labels and n_iter are equal under the asserted gap (the host path's smallest
relative gap between a row's two best keys, asked to exceed 1e-9, far above ASSIGN), the final centres are then UPDATE of
the same labels, and a row's min_s moves by at most 2 sqrt(min_s) |e_c| + |e_c|^2 with the centre error e_c on top of
ASSIGN; the inertia adds (n + 8) u inertia for its own sum.  The largest ratio to these bounds over the shapes of
test_whole_run was 0 (centres: with one row range the device's order of summation is the host's) and 0.0045
(inertia); of test_silhouette 0.034.
The silhouette: S(i, c) sums at most n square roots in two orders, each root within 1 ulp of the (D + 8) u / 2 relative
error of its argument: |S_dev - S_host| <= (n + 8) u S with D + 8 <= n + 8 folded in for the shapes here, and the
coefficient, 1 - a / b or b / a - 1 with the ratio at most 1, moves by at most 2 eps (1 + 2 eps), eps = (n + 8) u.

Shapes: 64 rows per workgroup block and 64 centres per LDS tile (n and k in 1, 63, 64, 65, 130 / 128), 32 columns per
staged chunk (D in 1, 2, 31, 32, 33, 128, 256), n = 70,000 rows with D = 4: more row blocks (1,094) than workgroups
(1,024) and more than one tile per row range of the sums; a padded row stride throughout."""
import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import cluster, cluster_ops as ops
from mmgnn.model import build_model
from mmgnn.synth import make_graph
import cluster_ref as cr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -53
MIN_GAP = 1e-9
B, K = ops.KM_ROW_TILE, ops.KM_MAX_K
assert (B, K, ops.KM_MAX_GRID, ops.KM_MAX_RANGES) == (64, 128, 1024, 128), "the shapes below are chosen for these switches"
BIG_N = 70000


def _padded(a, pad=3, fill=1e6):
    """A host matrix -> the view of the data inside a device buffer with `pad` more sentinel columns."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(DEV)
    return buf[:, :a.shape[1]]


def _centers(c):
    return torch.from_numpy(np.ascontiguousarray(c, np.float64)).to(DEV)


def _assign_case(kind, n, D, k, seed=0):
    if kind == "lattice":
        return cr.lattice(n, D, seed + 1), cr.lattice(k, D, seed + 2).astype(np.float64)
    x = cr.blobs(n, D, max(2, min(k, 8)), seed + 3)
    rs = np.random.RandomState(seed + 4)
    return x, x[rs.randint(n, size=k)].astype(np.float64) + rs.randn(k, D) * 0.5


ASSIGN_SHAPES = sorted({(n, 5, min(3, n)) for n in (1, 63, 64, 65, 130)}
                       | {(130, 5, k) for k in (1, 2, 63, 64, 65, 128)}
                       | {(130, D, 7) for D in (1, 2, 31, 32, 33, 128, 256)} | {(BIG_N, 4, 9)})


@pytest.mark.parametrize("n,D,k", ASSIGN_SHAPES)
@pytest.mark.parametrize("kind", ["lattice", "generic"])
def test_assign(kind, n, D, k):
    x, c = _assign_case(kind, n, D, k)
    hl, hs, gap = cluster.assign_host(x, c)
    changed = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    prev = torch.from_numpy(hl.copy()).to(DEV)
    prev[::3] = -1
    dl, ds = ops.km_assign(_padded(x), _centers(c), prev, None, None, changed)
    dl, ds = dl.cpu().numpy(), ds.cpu().numpy()
    if kind == "lattice":
        if k > 1 and D <= 5 and n >= 63:
            two = np.sort(cr.sqdist(x, c), axis=1)[:, :2]
            assert (two[:, 0] == two[:, 1]).any(), "the lattice case has no real tie"
        assert np.array_equal(dl, hl) and np.array_equal(ds, hs)
    else:
        assert k == 1 or gap > MIN_GAP, gap
        assert np.array_equal(dl, hl)
        assert np.all(np.abs(ds - hs) <= (D + 8) * U * hs)
    assert int(changed.item()) == len(range(0, n, 3))
    lab2, s2 = cluster.assign(_padded(x), c)                     # the public call
    assert np.array_equal(lab2.cpu().numpy(), hl) and np.array_equal(s2.cpu().numpy(), ds)


def _center_bound(x, labels, counts):
    """UPDATE per (cluster, column); 0 for a cluster without rows (it keeps its old centre on both sides)."""
    absum = np.zeros((counts.size, x.shape[1]))
    np.add.at(absum, labels, np.abs(x.astype(np.float64)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(counts[:, None] > 0, (counts[:, None] + 8) * U * absum / counts[:, None], 0.0)


def _update_both(x, c, labels=None, min_s=None):
    if labels is None:
        labels, min_s, _ = cluster.assign_host(x, c)
    h_new, h_counts, h_shift, h_m, h_rows = cluster.update_host(x, labels, min_s, c)
    changed = torch.tensor([17], dtype=torch.int64, device=DEV)
    rows = torch.full((c.shape[0],), -5, dtype=torch.int64, device=DEV)
    d_new, d_counts, status = ops.km_update(_padded(x), torch.from_numpy(labels).to(DEV), torch.from_numpy(min_s).to(DEV),
                                            _centers(c), None, None, changed, None, rows)
    d_new, d_counts, status, rows = d_new.cpu().numpy(), d_counts.cpu().numpy(), status.cpu().numpy(), rows.cpu().numpy()
    assert np.array_equal(d_counts, h_counts)
    assert status[0] == 17.0 and status[2] == h_m
    assert rows[:h_m].tolist() == h_rows.tolist() and np.all(rows[h_m:] == -1)
    # after relocation the rows of a cluster are not those of its label: bound with the larger, unrelocated set
    raw = np.bincount(labels, minlength=c.shape[0])
    bound = _center_bound(x, labels, np.maximum(raw, 1)) * np.maximum(raw, 1)[:, None] / np.maximum(h_counts, 1)[:, None]
    err = np.abs(d_new - h_new)
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    diff = np.abs(h_new - c)
    shift_bound = float((2 * diff * bound + bound ** 2).sum()) + (c.size + 8) * U * h_shift
    assert abs(status[1] - h_shift) <= shift_bound, (status[1], h_shift, shift_bound)
    return h_m, h_rows


@pytest.mark.parametrize("n,D,k", [(1, 3, 1), (65, 33, 2), (130, 31, 65), (1000, 128, 128), (3000, 256, 5), (BIG_N, 4, 9)])
def test_update(n, D, k):
    x, c = _assign_case("generic", n, D, k)
    _update_both(x, c)


@pytest.mark.parametrize("m", [1, 3])
def test_relocation_takes_the_hosts_rows(m):
    x = cr.blobs(500, 6, 4, seed=11)
    c = x[:4 + m].astype(np.float64).copy()
    for e in range(m):
        c[1 + 2 * e] = 1e3 * (e + 1)                             # empty clusters 1, 3, 5
    got_m, rows = _update_both(x, c)
    assert got_m == m and len(set(rows.tolist())) == m
    # ties in min_s: of equal keys the smaller row goes first
    xl = cr.lattice(300, 3, 5)
    cl = np.concatenate([cr.lattice(3, 3, 6).astype(np.float64), np.full((m, 3), 500.0) * (1 + np.arange(m))[:, None]])
    far = int(np.argmax(cluster.assign_host(xl, cl)[1]))
    xl[[7, 201]] = xl[far]                                       # three rows share the largest min_s
    labels, min_s, _ = cluster.assign_host(xl, cl)
    tied = np.flatnonzero(min_s == min_s.max())
    assert tied.size == 3
    _, rows = _update_both(xl, cl, labels, min_s)
    assert rows.tolist() == tied[:m].tolist()


def test_a_cluster_left_without_rows_keeps_its_centre():
    x = np.array([[0], [1], [10]], np.float32)
    labels, min_s = np.array([0, 0, 1], np.int32), np.array([0.25, 0.25, 4.0])
    c = np.array([[0.5], [8.0], [50.0]])
    new, counts, status = ops.km_update(torch.from_numpy(x).to(DEV), torch.from_numpy(labels).to(DEV),
                                        torch.from_numpy(min_s).to(DEV), _centers(c))
    assert counts.tolist() == [2, 0, 1] and new.cpu().numpy().tolist() == [[0.5], [8.0], [10.0]]
    assert status.tolist() == [0.0, 1600.0, 1.0]


RUN_SHAPES = [(65, 3, 2), (500, 16, 8), (3000, 2, 5), (1000, 32, 64), (2000, 128, 16)]


def _run_case(n, D, k):
    x = cr.blobs(n, D, k, seed=n)
    return x, cr.init_rows(x, k)


@pytest.mark.parametrize("n,D,k", RUN_SHAPES + [(400, 8, 5)])
def test_whole_run(n, D, k):
    if (n, D, k) == (400, 8, 5):                                 # one cluster empty in iteration 1
        x = cr.blobs(400, 8, 4, seed=7)
        init = x[:5].astype(np.float64).copy()
        init[2] = 1e3
    else:
        x, init = _run_case(n, D, k)
    h = cluster.kmeans(x, k, init=init)
    assert h.min_gap > MIN_GAP, h.min_gap
    # the labels the final centres were made from (after a strict stop: the final labels): UPDATE applies to them
    made_from, centers = None, init
    for _ in range(h.n_iter):
        made_from, s_from, _ = cluster.assign_host(x, centers)
        centers = cluster.update_host(x, made_from, s_from, centers)[0]
    assert np.array_equal(centers, h.cluster_centers)
    d = cluster.kmeans(_padded(x), k, init=init)
    assert d.cluster_centers.is_cuda and d.labels.is_cuda and d.labels.dtype == torch.int32
    assert np.array_equal(d.labels.cpu().numpy(), h.labels) and d.n_iter == h.n_iter and d.converged == h.converged
    assert np.array_equal(d.counts.cpu().numpy(), h.counts)
    cb = _center_bound(x, made_from, np.bincount(made_from, minlength=k))
    err = np.abs(d.cluster_centers.cpu().numpy() - h.cluster_centers)
    e2 = np.sqrt((cb ** 2).sum(axis=1))[h.labels]
    sb = (D + 8) * U * h.sqdist + 2 * np.sqrt(h.sqdist) * e2 + e2 ** 2
    ib = float(sb.sum()) + (n + 8) * U * h.inertia
    r_c = float((err / np.maximum(cb, 1e-300)).max())
    r_i = abs(d.inertia - h.inertia) / ib
    print(f"run {(n, D, k)}: n_iter {d.n_iter} centre error / bound {r_c:.3g} inertia error / bound {r_i:.3g}")
    assert np.all(err <= cb) and np.all(np.abs(d.sqdist.cpu().numpy() - h.sqdist) <= sb)
    assert abs(d.inertia - h.inertia) <= ib
    sd = d.sdist.cpu().numpy()
    assert np.allclose(sd, h.sdist, rtol=(n + 8) * U + float((sb / np.maximum(h.sqdist, 1e-300)).max()), atol=0)
    again = cluster.kmeans(_padded(x), k, init=init)
    for a, b in ((d.cluster_centers, again.cluster_centers), (d.labels, again.labels), (d.sqdist, again.sqdist),
                 (d.sdist, again.sdist)):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)), "two runs differ"
    assert d.inertia == again.inertia


def test_kmeans_plusplus_on_the_device_equals_the_host_draw():
    x = cr.blobs(700, 12, 6, seed=5)
    h, d = cluster.kmeans(x, 6, seed=3, n_init=2), cluster.kmeans(torch.from_numpy(x).to(DEV), 6, seed=3, n_init=2)
    assert h.min_gap > MIN_GAP
    assert np.array_equal(d.labels.cpu().numpy(), h.labels) and d.n_iter == h.n_iter
    assert abs(d.inertia - h.inertia) <= 1e-12 * h.inertia


def test_one_step_eager_equals_a_replayed_graph():
    n, D, k = 3000, 33, 65
    x, c0 = _assign_case("generic", n, D, k, seed=2)
    xd, c_start = _padded(x), _centers(c0)
    cen = torch.empty_like(c_start)
    labels = torch.empty(n, dtype=torch.int32, device=DEV)
    min_s = torch.empty(n, dtype=torch.float64, device=DEV)
    changed = torch.empty(1, dtype=torch.int64, device=DEV)
    counts = torch.empty(k, dtype=torch.int32, device=DEV)
    status = torch.empty(3, dtype=torch.float64, device=DEV)
    outs = (cen, labels, min_s, changed, counts, status)

    def reset():
        cen.copy_(c_start)
        for t in outs[1:]:
            t.fill_(-3)

    def run():
        ops.km_assign(xd, cen, labels, labels, min_s, changed)
        ops.km_update(xd, labels, min_s, cen, cen, counts, changed, status)

    def bits():
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in outs]

    reset()
    run()
    ref = bits()
    assert ref[3][0] == n and ref[5][1] > 0
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        reset()
        run()                                                    # warm-up off the default stream, as torch.cuda.graph asks
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        reset()
        graph.replay()
        for name, r, o in zip(("centres", "labels", "min_s", "changed", "counts", "status"), ref, bits()):
            assert np.array_equal(r.view(np.uint8), o.view(np.uint8)), f"{name}: a replayed capture differs from the eager run"


def _sil_split_n():
    """The smallest n = m B + 1 whose candidates are split into ranges."""
    return next(n for n in range(B + 1, 1 << 15, B) if ops.km_sil_plan(n)[0] > 1)


def _sil_labels(n, k, seed):
    labels = np.random.RandomState(seed).randint(0, k, size=n)
    labels[:k] = np.arange(k)                                    # every label occurs
    return labels.astype(np.int32)


@pytest.mark.parametrize("n,D,k", [(5, 3, 2), (64, 5, 2), (65, 33, 64), (300, 16, 128), (300, 128, 5), (None, 4, 7)])
def test_silhouette(n, D, k):
    n = _sil_split_n() if n is None else n
    x = cr.blobs(n, D, min(k, 6), seed=n + D)
    if n == 5:
        labels = np.array([0, 0, 1, 1, 1], np.int32)
    else:
        labels = _sil_labels(n, k, seed=k)
    if k == 128:
        assert (np.bincount(labels) == 1).any(), "no singleton cluster"
    host = cluster.silhouette_samples(x, labels)
    got = cluster.silhouette_samples(_padded(x), torch.from_numpy(labels).to(DEV))
    assert got.dtype == torch.float64 and got.is_cuda
    got = got.cpu().numpy()
    # S within (n + 8) u S, so a and b within eps = (n + 8) u relative; the coefficient is 1 - a / b or b / a - 1 with the
    # ratio at most 1, which moves by at most 2 eps (1 + 2 eps)
    eps = (n + 8) * U
    bound = 2 * eps * (1 + 2 * eps)
    err = np.abs(got - host)
    print(f"silhouette {(n, D, k)}: ranges {ops.km_sil_plan(n)[0]} error / bound {float(err.max() / bound):.3g}")
    assert np.all(err <= bound)
    counts = np.bincount(labels, minlength=k)
    assert np.all(got[counts[labels] == 1] == 0.0)
    q = np.array(sorted({0, n - 1, n // 2, min(n - 1, B), min(n - 1, B - 1)}))
    sub = cluster.silhouette_samples(_padded(x), torch.from_numpy(labels).to(DEV), queries=q).cpu().numpy()
    assert np.all(np.abs(sub - host[q]) <= bound)
    mean = cluster.silhouette_score(_padded(x), torch.from_numpy(labels).to(DEV))
    assert abs(mean - float(host.mean())) <= bound + (n + 8) * U
    sampled = cluster.silhouette_score(_padded(x), torch.from_numpy(labels).to(DEV), sample_size=max(2, n // 2), seed=1)
    assert abs(sampled - cluster.silhouette_score(x, labels, sample_size=max(2, n // 2), seed=1)) <= bound + (n + 8) * U


def test_scores_against_the_host():
    x, init = _run_case(500, 16, 8)
    h = cluster.kmeans(x, 8, init=init)
    xd = _padded(x)
    d = cluster.kmeans(xd, 8, init=init)
    hs, ds = cluster.cluster_scores(x, h), cluster.cluster_scores(xd, d)
    assert set(ds) == {"inertia", "davies_bouldin", "calinski_harabasz", "silhouette", "smallest_cluster"}
    for key in ("inertia", "davies_bouldin", "calinski_harabasz", "silhouette"):
        assert abs(ds[key] - hs[key]) <= 1e-12 * max(1.0, abs(hs[key])), key
    assert ds["smallest_cluster"] == hs["smallest_cluster"]
    assert abs(cluster.davies_bouldin(xd, d.labels) - hs["davies_bouldin"]) <= 1e-12
    assert abs(cluster.calinski_harabasz(xd, d.labels) - hs["calinski_harabasz"]) <= 1e-12 * hs["calinski_harabasz"]
    frame = cluster.k_sweep(xd, [2, 8], seed=0)
    assert list(frame.columns) == cluster.SWEEP_COLUMNS and frame["inertia"][0] > frame["inertia"][1]


def test_refusals_before_anything_is_enqueued():
    x = torch.zeros(10, 4, device=DEV)
    c = torch.zeros(2, 4, dtype=torch.float64, device=DEV)
    lib = ops.load()
    assert lib.mmg_km_assign_ws_bytes(10, 257, 2) == 0 and lib.mmg_km_update_ws_bytes(10, 4, 129) == 0
    assert lib.mmg_km_update_ws_bytes(10, 4, 11) == 0 and lib.mmg_km_silhouette_ws_bytes(10, 4, 10, 1) == 0
    assert lib.mmg_km_scores_ws_bytes(0, 2) == 0 and lib.mmg_km_colstats_ws_bytes(10, 0) == 0
    with pytest.raises(mmgnn._lib.MmgError, match="exceeds the 10 rows"):
        ops.km_assign(x, torch.zeros(11, 4, dtype=torch.float64, device=DEV))
    with pytest.raises(mmgnn._lib.MmgError, match="workspace"):
        ops._call("mmg_km_update", ops.ops._rows_matrix(x, "x")[0], 10, 4, 4, torch.zeros(10, dtype=torch.int32, device=DEV),
                  torch.zeros(10, dtype=torch.float64, device=DEV), c, 2, c.clone(), torch.zeros(2, dtype=torch.int32, device=DEV),
                  None, torch.zeros(3, dtype=torch.float64, device=DEV), None)
    with pytest.raises(TypeError, match="torch.float32"):
        cluster.kmeans(x.double(), 2)


@pytest.mark.parametrize("n,D", [(1, 1), (65, 33), (BIG_N, 4)])
def test_colstats(n, D):
    """Column means within (n + 8) u sum|x| / n; the one-pass variance sum x^2 / n - mean^2 within (n + 8) u of each of its
    two terms (+ the error of the mean, 2 |mean| times its bound)."""
    x = cr.blobs(n, D, 3, seed=1)
    x64 = x.astype(np.float64)
    mean, var = ops.km_colstats(_padded(x))
    mb = (n + 8) * U * np.abs(x64).mean(axis=0)
    assert np.all(np.abs(mean.cpu().numpy() - x64.mean(axis=0)) <= mb)
    m2 = (x64 ** 2).mean(axis=0)
    vb = (n + 8) * U * (m2 + x64.mean(axis=0) ** 2) + 2 * np.abs(x64.mean(axis=0)) * mb + mb ** 2
    assert abs(float(var.item()) - float(x64.var(axis=0).mean())) <= float(vb.mean()) + 8 * U * float(x64.var(axis=0).mean())


@pytest.fixture(scope="module")
def model_and_graph():
    g = make_graph(1, seed=0).to(DEV)
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"}}
    torch.manual_seed(0)
    model = build_model(cfg, (g.node_types, g.edge_types), None).to(DEV)
    model._init_embeddings(g)
    model.train()
    return model, g


def test_patient_and_lab_clusters(model_and_graph, tmp_path):
    model, g = model_and_graph
    out = cluster.patient_clusters(model, g, n_clusters=4, space="initial", seed=1, output_dir=tmp_path, sample_size=512)
    n, e = int(g["patient"].num_nodes), int(g[("patient", "has_lab", "lab")].edge_index.shape[1])
    import pandas as pd
    pat, summ, prof = (pd.read_csv(tmp_path / f) for f in ("patient_clusters.csv", "cluster_summary.csv", "cluster_lab_profile.csv"))
    assert list(pat.columns) == cluster.PATIENT_CLUSTER_COLUMNS and len(pat) == n
    assert list(summ.columns) == cluster.CLUSTER_SUMMARY_COLUMNS and len(summ) == 4
    assert list(prof.columns) == cluster.LAB_PROFILE_COLUMNS
    assert int(summ["n_patients"].sum()) == n and int(prof["n_observed"].sum()) == e
    assert np.array_equal(np.bincount(pat["cluster"], minlength=4), summ["n_patients"].to_numpy())
    assert float(prof["coverage"].max()) <= 1.0 + 1e-12 and np.all(pat["distance"] >= 0)
    labs = cluster.lab_clusters(model, g, n_clusters=3, output_dir=tmp_path)
    lab, table = pd.read_csv(tmp_path / "lab_clusters.csv"), pd.read_csv(tmp_path / "lab_cluster_panel_table.csv")
    assert list(lab.columns) == cluster.LAB_CLUSTER_COLUMNS and len(lab) == int(g["lab"].num_nodes)
    assert table.columns[0] == "cluster" and int(table.drop(columns="cluster").to_numpy().sum()) == len(lab)
    assert int(labs["result"].counts.sum().item()) == len(lab)
