"""Nearest-neighbour imputation on the MI355X: mmg_knn_impute against the float64 restatement (knn_ref.py) over lab
counts, neighbour counts, weights, sizes and densities; request handling; bitwise reproducibility; the x100 eICU shape;
and evaluate_nearest_neighbor_baseline."""
import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import ops
from mmgnn.knn import KNNLabImputer
from knn_ref import knn_impute_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5


def _matrix(seed, N, L, density):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, L)).astype(np.float32)
    X[rng.random((N, L)) >= density] = np.nan
    if N > 2:
        X[1] = np.nan                                        # a row with no observed value
    if L > 2:
        X[:, L - 2] = np.nan                                 # a lab nobody has
    return X


def _compare(got, X, rows, k, weights):
    """got [len(rows), L] from the kernel vs the restatement: 1e-5 abs + rel per cell; a mismatch is exempt only at a
    near tie of the selection (k'-th and (k'+1)-th distances within 1e-5 relative), and those must be <= 0.1 %."""
    want, gap = knn_impute_ref(X.astype(np.float64), rows=rows, k=k, weights=weights, return_gap=True)
    got = np.asarray(got, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"NaN pattern differs in {int((np.isnan(got) != np.isnan(want)).sum())} cells"
    fin = ~np.isnan(want)
    bad = np.zeros(want.shape, bool)
    bad[fin] = np.abs(got[fin] - want[fin]) > TOL + TOL * np.abs(want[fin])
    exempt = bad & (gap <= TOL)
    hard = bad & ~exempt
    assert not hard.any(), (f"{int(hard.sum())} cells off (max {np.abs(got - want)[hard].max():.3g}); "
                            f"{int(exempt.sum())} near-tie cells exempt")
    assert exempt.sum() <= 1e-3 * want.size, f"{int(exempt.sum())} of {want.size} cells exempt as near ties"


CASES = [  # N, L, density, k, weights
    (1, 12, 0.5, 5, "uniform"),
    (2, 12, 0.6, 1, "distance"),
    (300, 1, 0.5, 5, "uniform"),
    (300, 12, 0.05, 32, "distance"),
    (300, 50, 0.3, 5, "uniform"),
    (300, 50, 0.7, 5, "distance"),
    (1834, 50, 0.47, 5, "uniform"),
    (1834, 50, 0.47, 5, "distance"),
    (1834, 64, 0.95, 32, "uniform"),
    (1834, 65, 0.5, 1, "distance"),
    (300, 300, 0.05, 5, "uniform"),      # more missing cells than a workgroup's lanes: two passes
    (300, 300, 0.6, 32, "distance"),
    (300, 512, 0.5, 32, "uniform"),
    (300, 512, 0.2, 1, "distance"),
    (5000, 50, 0.47, 5, "uniform"),
    (5000, 12, 0.95, 32, "distance"),
    (5000, 65, 0.15, 1, "uniform"),
]


@pytest.mark.parametrize("N,L,density,k,weights", CASES)
def test_kernel_matches_the_restatement(N, L, density, k, weights):
    X = _matrix(N * 7 + L, N, L, density)
    Xd = torch.from_numpy(X).to(DEV)
    rows = np.arange(N) if N <= 2000 else np.random.default_rng(N).choice(N, 200, replace=False)
    got = ops.knn_impute(Xd, torch.from_numpy(rows.astype(np.int32)).to(DEV), k, weights)
    _compare(got.cpu().numpy(), X, rows, k, weights)


def test_requests_subsets_repeats_empty_and_out_of_range():
    X = _matrix(3, 500, 50, 0.4)
    Xd = torch.from_numpy(X).to(DEV)
    full = ops.knn_impute(Xd, torch.arange(500, dtype=torch.int32, device=DEV), 5, "distance").cpu()
    rows = torch.tensor([7, 3, 7, -1, 499, 500, 2 ** 31 - 1, 0, 3], dtype=torch.int32)
    out = torch.full((rows.numel(), 57), 7.25, dtype=torch.float32, device=DEV)      # ld_out > n_cols
    ops.knn_impute(Xd, rows.to(DEV), 5, "distance", out=out)
    out = out.cpu()
    valid = (rows >= 0) & (rows < 500)
    assert torch.equal(out[valid, :50].view(torch.int32), full[rows[valid].long()].view(torch.int32))
    assert torch.all(out[~valid] == 7.25)                     # skipped rows untouched
    assert torch.all(out[:, 50:] == 7.25)                     # padding columns untouched
    empty = ops.knn_impute(Xd, torch.empty(0, dtype=torch.int32, device=DEV), 5)
    assert empty.shape == (0, 50)


def test_wrapper_refuses_wrong_device_and_dtype():
    X = torch.from_numpy(_matrix(4, 50, 12, 0.5))
    r = torch.arange(50, dtype=torch.int32)
    with pytest.raises(Exception, match="HIP device"):
        ops.knn_impute(X, r.to(DEV), 5)
    with pytest.raises(Exception, match="HIP device"):
        ops.knn_impute(X.to(DEV), r, 5)
    with pytest.raises(TypeError):
        ops.knn_impute(X.double().to(DEV), r.to(DEV), 5)
    with pytest.raises(TypeError):
        ops.knn_impute(X.to(DEV), r.long().to(DEV), 5)
    with pytest.raises(ValueError, match="weights"):
        ops.knn_impute(X.to(DEV), r.to(DEV), 5, "gaussian")
    with pytest.raises(Exception, match="n_neighbors"):
        ops.knn_impute(X.to(DEV), r.to(DEV), 33)


@pytest.mark.parametrize("L,k", [(50, 5), (300, 32)])
def test_bitwise_reproducible_and_independent_of_the_request(L, k):
    N = 1500
    Xd = torch.from_numpy(_matrix(5 + L, N, L, 0.5)).to(DEV)
    all_rows = torch.arange(N, dtype=torch.int32, device=DEV)
    a = ops.knn_impute(Xd, all_rows, k, "distance")
    b = ops.knn_impute(Xd, all_rows, k, "distance")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for r in (0, 2, 777, N - 1):
        one = ops.knn_impute(Xd, torch.tensor([r], dtype=torch.int32, device=DEV), k, "distance")
        assert torch.equal(one[0].view(torch.int32), a[r].view(torch.int32)), r
    sub = torch.tensor([N - 1, 5, 900], dtype=torch.int32, device=DEV)
    c = ops.knn_impute(Xd, sub, k, "distance")
    assert torch.equal(c.view(torch.int32), a[sub.long()].view(torch.int32))


def _train_split(scale):
    from mmgnn import synth
    from mmgnn.train import EdgeMasker
    g = synth.make_graph(scale, device=DEV)
    masker = EdgeMasker(g)
    return g, masker


def test_x100_eicu_shape_sampled_receivers():
    g, masker = _train_split(100)
    ei, ev, _, _ = masker.get_masked_data("train", want_mask=False)
    imp = KNNLabImputer(5, "uniform").fit(ei[0], ei[1], ev, g["patient"].num_nodes, g["lab"].num_nodes)
    X = imp.X.cpu().numpy()
    assert X.shape == (183400, 50)
    rows = np.sort(np.random.default_rng(11).choice(X.shape[0], 256, replace=False))
    got = imp.impute_matrix(torch.from_numpy(rows).to(DEV)).cpu().numpy()
    _compare(got, X, rows, 5, "uniform")
    # predict() gathers the same cells
    lab = torch.arange(50, device=DEV).repeat(4)
    pat = torch.from_numpy(np.repeat(rows[:4], 50)).to(DEV)
    assert torch.equal(imp.predict(pat, lab).cpu(), torch.from_numpy(got[:4].reshape(-1)))


@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_evaluate_nearest_neighbor_baseline(weights):
    from mmgnn.evaluate import compute_regression_metrics, evaluate_nearest_neighbor_baseline
    g, masker = _train_split(1)
    res = evaluate_nearest_neighbor_baseline(g, masker, split="test", n_neighbors=5, weights=weights)
    assert set(res) == {"nearest_neighbor"}
    tr_ei, tr_v, _, _ = masker.get_masked_data("train", want_mask=False)
    te_ei, te_v, _, _ = masker.get_masked_data("test", want_mask=False)
    P, L = g["patient"].num_nodes, g["lab"].num_nodes
    X = np.full((P, L), np.nan)
    tp, tl = tr_ei.cpu().numpy()
    X[tp, tl] = tr_v.cpu().numpy()
    p, lab = te_ei.cpu().numpy()
    uniq, inv = np.unique(p, return_inverse=True)
    pred = knn_impute_ref(X, rows=uniq, k=5, weights=weights)[inv, lab]
    pred = np.where(np.isnan(pred), np.mean(tr_v.cpu().numpy()), pred).astype(np.float32)
    want = compute_regression_metrics(pred, te_v.cpu().numpy())
    for key in ("mae", "rmse", "r2", "mape"):
        assert res["nearest_neighbor"][key] == pytest.approx(want[key], rel=1e-6, abs=1e-6), key
