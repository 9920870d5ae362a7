"""CPU-side checks of nearest-neighbour imputation (no GPU): the float64 restatement in knn_ref.py equals
sklearn.impute.KNNImputer, the exact-zero-distance rule, the C-ABI entry point's declaration and host-side argument
errors, and KNNLabImputer.fit's input validation."""
import ctypes
import os

import numpy as np
import pytest
import torch

from knn_ref import knn_impute_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _matrix(seed, N, L, density, empty_rows=2, empty_col=True):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, L))
    X[rng.random((N, L)) >= density] = np.nan
    X[:empty_rows] = np.nan                                  # rows with no observed value
    if empty_col:
        X[:, L // 2] = np.nan                                # an all-missing column
    return X


def _sklearn(X, k, weights):
    from sklearn.impute import KNNImputer
    got = KNNImputer(n_neighbors=k, weights=weights).fit_transform(X)
    keep = ~np.all(np.isnan(X), axis=0)                      # sklearn drops the all-missing columns: put them back
    full = np.full(X.shape, np.nan)
    full[:, keep] = got
    return full


@pytest.mark.parametrize("k", [1, 3, 5, 32])
@pytest.mark.parametrize("weights", ["uniform", "distance"])
@pytest.mark.parametrize("N,L,density", [(40, 7, 0.5), (120, 12, 0.3), (60, 9, 0.15)])
def test_restatement_equals_sklearn(k, weights, N, L, density):
    pytest.importorskip("sklearn")
    X = _matrix(1000 * k + N, N, L, density)
    want = _sklearn(X, k, weights)
    got = knn_impute_ref(X, k=k, weights=weights)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    # (the all-NaN-distance fallback is the column mean rounded to fp32, as the kernel returns it; sklearn keeps fp64)
    np.testing.assert_allclose(got, want, rtol=1e-7, atol=1e-7, equal_nan=True)


def test_restatement_covers_the_special_cases():
    pytest.importorskip("sklearn")
    # lab 0 has 2 donors (k > |D_l|); row 2 shares no lab with either donor of lab 1 (all distances NaN -> column mean)
    nan = np.nan
    X = np.array([[1.0, nan, 2.0, nan],
                  [3.0, 5.0, nan, nan],
                  [nan, nan, nan, 4.0],
                  [nan, 7.0, 1.0, nan],
                  [nan, nan, nan, nan]])
    for weights in ("uniform", "distance"):
        got = knn_impute_ref(X, k=5, weights=weights)
        np.testing.assert_allclose(got, _sklearn(X, 5, weights), rtol=1e-7, equal_nan=True)
        assert got[2, 1] == np.float32(6.0) and got[2, 0] == np.float32(2.0)     # the column means
        assert np.all(got[[0, 1, 3, 4], 3] == 4.0)          # lab 3's only donor shares no lab with anyone


def test_exact_zero_distance_weights():
    nan = np.nan
    # row 0's neighbours for lab 2: row 1 (identical on the common labs: distance exactly 0), rows 2 and 3 farther
    X = np.array([[1.0, 2.0, nan],
                  [1.0, 2.0, 10.0],
                  [1.5, 2.0, 20.0],
                  [1.0, 3.0, 40.0],
                  [nan, 2.0, 30.0]])            # row 4 shares lab 1 with row 0 at distance 0 as well
    got = knn_impute_ref(X, rows=[0], k=3, weights="distance")
    assert got[0, 2] == 20.0                    # only the zero-distance donors: mean(10, 30)
    got = knn_impute_ref(X, rows=[0], k=1, weights="distance")
    assert got[0, 2] == 10.0                    # tie at 0 -> the lower row index
    got = knn_impute_ref(X, rows=[0], k=3, weights="uniform")
    assert got[0, 2] == pytest.approx((10.0 + 30.0 + 20.0) / 3)
    # no zero among the chosen: 1 / dist weights, dist = sqrt(L * S / c)
    Y = X[[0, 2, 3]]
    d2, d3 = np.sqrt(3 * 0.25 / 2), np.sqrt(3 * 1.0 / 2)
    got = knn_impute_ref(Y, rows=[0], k=2, weights="distance")
    assert got[0, 2] == pytest.approx((20.0 / d2 + 40.0 / d3) / (1 / d2 + 1 / d3), rel=1e-12)


def test_entry_point_is_declared_and_prototyped():
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    _lib.load()
    hdr = open(os.path.join(REPO, "include", "mmgnn.h")).read()
    assert "mmg_knn_impute(" in hdr and "mmg_knn_impute_ws_bytes(" in hdr
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mmg_knn_impute")
    res, args = _lib.SIGNATURES["mmg_knn_impute"]
    assert res is ctypes.c_int and len(args) == 13


def test_argument_errors_are_reported_without_a_gpu():
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(256)                 # never dereferenced: every call below fails on the host
    need = lib.mmg_knn_impute_ws_bytes(100, 50, 10, 5)
    assert need >= 50 * 4

    def call(N=100, L=50, ld_x=50, n_out=10, k=5, w=0, ld_out=50, ws_bytes=need, X=fake, rows=fake, out=fake, ws=fake):
        return lib.mmg_knn_impute(X, N, L, ld_x, rows, n_out, k, w, out, ld_out, ws, ws_bytes, None)

    def err():
        return lib.mmg_last_error().decode()

    assert call(k=0) == -1 and "n_neighbors" in err()
    assert call(k=33) == -1 and "n_neighbors" in err()
    assert call(L=0, ld_x=0, ld_out=0) == -1 and "n_cols" in err()
    assert call(L=513, ld_x=513, ld_out=513) == -1 and "n_cols" in err()
    assert call(w=2) == -1 and "weights" in err()
    assert call(ld_x=49) == -1 and "ld_x" in err()
    assert call(ld_out=49) == -1 and "ld_out" in err()
    assert call(N=1 << 31) == -1 and "n_rows" in err()
    assert call(n_out=-1) == -1 and "n_out" in err()
    assert call(ws_bytes=need - 1) == -3 and "workspace" in err()
    assert call(ws=None) == -3 and "workspace" in err()
    assert call(rows=None) == -1 and "null buffer" in err()
    assert call(n_out=0) == 0                   # an empty request enqueues nothing


def test_fit_validates_its_input():
    import mmgnn  # noqa: F401
    from mmgnn.knn import KNNLabImputer
    p = torch.tensor([0, 1, 2, 1])
    lab = torch.tensor([0, 1, 2, 1])
    v = torch.tensor([0.5, 1.0, -1.0, 2.0])
    with pytest.raises(ValueError, match="duplicate"):
        KNNLabImputer().fit(p, lab, v, 3, 3)
    with pytest.raises(ValueError, match="NaN"):
        KNNLabImputer().fit(p[:3], lab[:3], torch.tensor([0.5, float("nan"), 1.0]), 3, 3)
    with pytest.raises(ValueError, match="patient index"):
        KNNLabImputer().fit(p[:3], lab[:3], v[:3], 2, 3)
    with pytest.raises(ValueError, match="lab index"):
        KNNLabImputer().fit(p[:3], lab[:3], v[:3], 3, 2)
    with pytest.raises(ValueError, match="n_labs"):
        KNNLabImputer().fit(p[:3], lab[:3], v[:3], 3, 513)
    with pytest.raises(ValueError, match="n_neighbors"):
        KNNLabImputer(n_neighbors=33).fit(p[:3], lab[:3], v[:3], 3, 3)
    with pytest.raises(ValueError, match="weights"):
        KNNLabImputer(weights="gaussian").fit(p[:3], lab[:3], v[:3], 3, 3)
    with pytest.raises(Exception, match="HIP device"):
        KNNLabImputer().fit(p[:3], lab[:3], v[:3], 3, 3)   # valid, but on the host: no CPU fallback
