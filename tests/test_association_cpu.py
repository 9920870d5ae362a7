"""Lab association without a GPU: the numpy restatement of mmgnn/association.py against the loop reference
(tests/assoc_ref.py: fsum sums, 80-bit finish) and against pandas.DataFrame.corr / .cov(min_periods=) with pandas' own
distance from that reference as the yardstick; the binding of libmmgnn_assoc.so from its header; the drivers on a small
synthetic graph through the numpy path."""
import ctypes
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import _lib, ops
from mmgnn import association as asc
from mmgnn.synth import make_graph
import assoc_ref as ref

F32 = np.float32

SHAPES, case = ref.PANDAS_SHAPES, ref.pandas_case


def nan_equal(a, b):
    return bool(np.array_equal(np.isnan(a), np.isnan(b)))


# ---------------------------------------------------------------------------------- restatement against the loop reference
@pytest.mark.parametrize("n, L, density, mp, seed", SHAPES)
def test_restatement_against_the_loop_reference(n, L, density, mp, seed):
    X = case(n, L, density, seed)
    mom = asc.pairwise_moments(X)
    count, s, sa, n_inf = ref.colstats(X)
    assert n_inf == 0 and np.array_equal(mom.count, count) and mom.count.dtype == np.int64
    mean_ref = np.divide(s, count, out=np.zeros(L), where=count > 0)
    assert np.all(np.abs(mom.center * count - s) <= (count + 8) * ref.U * sa)
    assert mom.center[1] == 0.0 and mom.center[2] == 2.5                    # nobody has lab 1; lab 2 is constant
    assert np.allclose(mom.center, mean_ref, rtol=1e-14, atol=0)
    want, ab = ref.moments(X, mom.center)
    assert np.array_equal(mom.planes[0], want[0])
    err = np.abs(mom.planes - want)
    assert np.all(err <= ref.moment_bound(ab)), float((err / np.maximum(ref.moment_bound(ab), 1e-300)).max())
    got = asc.lab_correlation(X, mp)
    r, cov, jac, lift = ref.finish(want, count, n, mp)
    assert np.array_equal(got.n, want[0].astype(np.int64)) and got.n_rows == n
    assert np.array_equal(got.jaccard, jac, equal_nan=True) and np.array_equal(got.lift, lift, equal_nan=True)
    assert nan_equal(got.r, r) and nan_equal(got.cov, cov)
    # the special cells: 0, 1 and 2 common rows
    assert (want[0, 4, 5], want[0, 3, 4], want[0, 3, 5]) == (0, 1, 2)
    assert np.isnan(got.r[2]).all() and np.isnan(got.r[1]).all() and np.isnan(got.cov[3, 4])
    if mp <= 2:
        assert abs(got.r[3, 5]) == 1.0 and np.isfinite(got.cov[3, 5])
    else:
        assert np.isnan(got.r[3, 5]) and np.isnan(np.diagonal(got.r)[want[0].diagonal() < mp]).all()


def test_exact_on_lattice_inputs_and_independent_of_the_centre():
    X = ref.make_matrix(700, 9, 11, 0.5, lattice=True)
    c = ref.lattice_center(9, 11)
    mom = asc.pairwise_moments(X, c)
    want, _ = ref.moments(X, c)
    assert np.array_equal(mom.planes, want) and np.array_equal(mom.center, c)
    a = asc.host_finish(mom.planes, mom.count, 700, 1)
    b = asc.host_finish(asc.pairwise_moments(X).planes, mom.count, 700, 1)
    for x, y in zip(a[:2], b[:2]):
        assert nan_equal(x, y) and np.allclose(x, y, rtol=0, atol=1e-12, equal_nan=True)


def test_an_infinite_cell_and_bad_shapes_are_refused():
    X = ref.make_matrix(20, 6, 0)
    X[5, 0] = np.inf
    with pytest.raises(ValueError, match="1 infinite"):
        asc.lab_correlation(X)
    with pytest.raises(ValueError, match="labs"):
        asc.lab_correlation(np.zeros((4, 513), F32))
    with pytest.raises(ValueError, match="2-D"):
        asc.lab_correlation(np.zeros(4, F32))
    with pytest.raises(ValueError, match="min_periods"):
        asc.lab_correlation(np.zeros((4, 3), F32), -1)


# ---------------------------------------------------------------------------------- restatement against pandas
@pytest.mark.parametrize("n, L, density, mp, seed", SHAPES)
def test_restatement_against_pandas(n, L, density, mp, seed):
    """The NaN pattern EQUALS pandas'; the values are at most 8 x as far from the loop reference (fsum moments about the
    column means, 80-bit finish) as pandas' own corr / cov are -- the largest distance over the table; covariances relative
    to sqrt(cov_aa cov_bb) of the reference."""
    X = case(n, L, density, seed)
    frame = pd.DataFrame(X.astype(np.float64))
    p_r, p_cov = frame.corr(min_periods=mp).to_numpy(), frame.cov(min_periods=mp).to_numpy()
    got = asc.lab_correlation(X, mp)
    assert nan_equal(got.r, p_r), "corr: NaN pattern"
    assert nan_equal(got.cov, p_cov), "cov: NaN pattern"
    count, _, _, _ = ref.colstats(X)
    want, _ = ref.moments(X, got.mean)
    r, cov, _, _ = ref.finish(want, count, n, mp)
    assert nan_equal(r, p_r) and nan_equal(cov, p_cov)
    assert np.isfinite(r[~np.eye(L, dtype=bool)]).any() and (mp == 1 or np.isnan(r[want[0] > 0]).any())
    _, cov1, _, _ = ref.finish(want, count, n, 1)
    with np.errstate(invalid="ignore"):
        scale = np.sqrt(np.abs(np.outer(np.diagonal(cov1), np.diagonal(cov1))))
    scale = np.where(np.isfinite(scale) & (scale > 0), scale, 1.0)
    dist = lambda x, y, s=1.0: float(np.nanmax(np.abs(x - y) / s, initial=0.0))          # noqa: E731
    d_r, dp_r = dist(got.r, r), dist(p_r, r)
    d_c, dp_c = dist(got.cov, cov, scale), dist(p_cov, cov, scale)
    print(f"({n}, {L}, {density}, mp {mp}): r restatement {d_r:.2e} pandas {dp_r:.2e}; cov restatement {d_c:.2e} "
          f"pandas {dp_c:.2e}")
    assert d_r <= 8 * dp_r and d_c <= 8 * dp_c
    assert np.array_equal(got.n, frame.notna().to_numpy().astype(np.int64).T @ frame.notna().to_numpy().astype(np.int64))


# ---------------------------------------------------------------------------------- the binding
def test_the_assoc_header_parses_and_names_what_the_library_defines():
    from mmgnn import assoc_ops as m
    b = m.BINDING
    assert isinstance(b, _lib.Binding) and b.stem == "assoc"
    assert os.path.basename(b.lib_path) == "libmmgnn_assoc.so" and os.path.basename(b.header_path) == "mmgnn_assoc.h"
    assert (m.DEFINES, m.SIGNATURES, m.PARAMS) == (b.defines, b.signatures, b.params)
    text = re.sub(r"/\*.*?\*/", "", open(b.header_path).read(), flags=re.S)
    assert sorted(re.findall(r"^\s*#\s*define\s+(MMG_\w+)", text, flags=re.M)) == sorted(b.defines) and b.defines
    for name, v in b.defines.items():
        assert type(v) is int and getattr(m, name) == v
    assert m.AS_MAX_LABS == asc.MAX_LABS == 512
    assert not set(b.signatures) & set(_lib.SIGNATURES)
    assert os.path.exists(b.lib_path), f"{b.lib_path} is not built (make -C multi-modal-gnn_amd/csrc)"
    ctypes.CDLL(_lib.LIB_PATH, mode=ctypes.RTLD_GLOBAL)               # the satellite links against it
    raw = ctypes.CDLL(b.lib_path)
    for sym in b.signatures:
        assert hasattr(raw, sym), sym
    assert sorted(b.signatures) == sorted(
        f"mmg_assoc_{s}" for s in ("plan", "colstats", "colstats_ws_bytes", "moments", "moments_ws_bytes", "finish",
                                   "finish_ws_bytes"))
    with_ws = [sym for sym, params in b.params.items() if any(p[0] == "ws" for p in params)]
    assert sorted(with_ws) == ["mmg_assoc_colstats", "mmg_assoc_finish", "mmg_assoc_moments"]
    for sym in with_ws:
        assert sym + "_ws_bytes" in b.signatures and b.signatures[sym + "_ws_bytes"][0] is ctypes.c_size_t, sym
        assert [p[0] for p in b.params[sym]][-3:] == ["ws", "ws_bytes", "stream"], sym
        assert b.params[sym][-3][1:] == ("void", 1) and b.params[sym][-2][1:] == ("size_t", 0), sym
    assert sorted(ops._plans(b)) == sorted(b.signatures)


def test_the_plan_and_the_host_refusals_of_the_library():
    """mmg_assoc_plan and every argument check run on the host: no device is needed (null device pointers are refused
    after the shape)."""
    from mmgnn import assoc_ops as m
    lib = m.load()
    for n, L in ((1, 1), (255, 50), (256, 50), (257, 50), (183400, 50), (183400, 512), (2 ** 31 - 2, 512), (5000, 130)):
        rows, slabs = m.assoc_plan(n, L)
        nb = (L + m.AS_TILE - 1) // m.AS_TILE
        target = m.MMG_AS_BLOCKS // (nb * (nb + 1) // 2)
        want = max(m.MMG_AS_MIN_ROWS, -(-(-(-n // target)) // m.AS_CHUNK) * m.AS_CHUNK)
        assert rows == want and rows % m.AS_CHUNK == 0 and slabs == -(-n // rows)
        assert lib.mmg_assoc_moments_ws_bytes(n, L) >= slabs * 4 * L * L * 8
        assert lib.mmg_assoc_colstats_ws_bytes(n, L) > 0
    for n, L in ((0, 5), (2 ** 31 - 1, 5), (10, 0), (10, 513)):
        assert lib.mmg_assoc_moments_ws_bytes(n, L) == 0 and lib.mmg_assoc_colstats_ws_bytes(n, L) == 0
        with pytest.raises(_lib.MmgError, match="assoc_plan"):
            m.assoc_plan(n, L)
    E_ARG, E_WS = _lib.MMG_E_ARG, _lib.MMG_E_WS
    assert lib.mmg_assoc_moments(None, 10, 0, 8, None, None, None, 0, None) == E_ARG
    assert lib.mmg_assoc_moments(None, 10, 513, 600, None, None, None, 0, None) == E_ARG
    assert lib.mmg_assoc_moments(None, 10, 8, 7, None, None, None, 0, None) == E_ARG
    assert b"ld_x 7 < L 8" in _lib.load().mmg_last_error()
    assert lib.mmg_assoc_moments(None, 10, 8, 8, None, None, None, 0, None) == E_ARG          # null pointers
    assert lib.mmg_assoc_colstats(None, 0, 8, 8, None, None, None, None, 0, None) == E_ARG
    assert lib.mmg_assoc_finish(None, None, 513, 10, 1, None, None, None, None, None, 0, None) == E_ARG
    assert lib.mmg_assoc_finish(None, None, 5, 10, -1, None, None, None, None, None, 0, None) == E_ARG
    assert E_ARG != E_WS


# ---------------------------------------------------------------------------------- frames and drivers
def test_the_fisher_interval_matches_a_hand_value():
    """r = 0.5 over n = 28 rows: z = atanh(0.5) = 0.549306144334, half width 1.959963984540 / sqrt(25) = 0.391992796908;
    tanh(0.157313347426) = 0.156028363, tanh(0.941298941242) = 0.735818479."""
    lo, hi = asc.fisher_interval(0.5, 28)
    assert abs(float(lo) - 0.156028363) < 1e-9 and abs(float(hi) - 0.735818479) < 1e-9
    assert abs(float(lo) - math.tanh(math.atanh(0.5) - 1.959963984540054 / 5)) < 1e-15
    lo, hi = asc.fisher_interval(np.array([0.3, 0.3, 1.0, -1.0, np.nan]), np.array([3, 4, 50, 50, 50]))
    assert np.isnan(lo[0]) and np.isnan(hi[0]) and lo[1] < 0.3 < hi[1]
    assert (lo[2], hi[2], lo[3], hi[3]) == (1.0, 1.0, -1.0, -1.0) and np.isnan(lo[4])


def test_pairs_are_sorted_by_absolute_r_then_by_index():
    L = 5
    r = np.full((L, L), np.nan)
    n = np.full((L, L), 40, np.int64)
    for (a, b), v in {(0, 1): 0.2, (0, 2): -0.9, (0, 3): 0.5, (1, 2): -0.5, (1, 3): 0.9, (2, 3): np.nan, (0, 4): 0.5}.items():
        r[a, b] = r[b, a] = v
    n[1, 4] = n[4, 1] = 29                                   # below min_periods: no row
    a = asc.LabAssociation(n, r, r, np.full((L, L), 0.5), np.ones((L, L)), np.full(L, 40), np.zeros(L), 100)
    f = asc.association_pairs(a, names=list("abcde"), min_periods=30)
    assert list(f.columns) == asc.PAIR_COLUMNS == ["lab_a", "lab_b", "n", "jaccard", "lift", "r", "r_lower", "r_upper"]
    assert list(zip(f.lab_a, f.lab_b)) == [("a", "c"), ("b", "d"), ("a", "d"), ("a", "e"), ("b", "c"), ("a", "b"), ("c", "d"),
                                           ("c", "e"), ("d", "e")]
    assert f.n.dtype == np.int64 and np.isnan(f.r.iloc[-1]) and np.isnan(f.r_lower.iloc[-1])
    assert f.r_lower.iloc[0] < -0.9 < f.r_upper.iloc[0]
    assert len(asc.association_pairs(a, min_periods=41)) == 0 and asc.association_pairs(a, min_periods=0).lab_a[0] == "Lab_0"


def test_lab_matrix_validates_like_the_knn_imputer():
    p, l, v = np.array([0, 0, 2]), np.array([0, 1, 1]), np.array([1.0, 2.0, 3.0], F32)
    X = asc.lab_matrix(p, l, v, 3, 2)
    assert isinstance(X, np.ndarray) and X.dtype == F32
    assert np.array_equal(X, np.array([[1, 2], [np.nan, np.nan], [np.nan, 3]], F32), equal_nan=True)
    assert np.array_equal(asc.lab_matrix(torch.tensor(p), torch.tensor(l), torch.tensor(v)[:, None], 3, 2), X, equal_nan=True)
    for args, msg in (((p, l, v, 3, 513), "n_labs"), ((p, l, v, 0, 2), "n_patients"), ((p, l, v, 2, 2), "patient index"),
                      ((p, l, v, 3, 1), "lab index"), ((p, l, v[:2], 3, 2), "one entry per cell"),
                      ((p.astype(np.float64), l, v, 3, 2), "integers"), ((p, l, np.array([1, np.nan, 3], F32), 3, 2), "NaN"),
                      ((np.array([0, 0, 2]), np.array([1, 1, 1]), v, 3, 2), "duplicate")):
        with pytest.raises(ValueError, match=msg):
            asc.lab_matrix(*args)


def test_lab_association_on_a_synthetic_graph_through_the_numpy_path(tmp_path):
    g = make_graph(1, seed=0)
    assoc, frames = asc.lab_association(g, output_dir=tmp_path, min_periods=30)
    P, L = int(g["patient"].num_nodes), int(g["lab"].num_nodes)
    assert isinstance(assoc.r, np.ndarray) and assoc.r.shape == (L, L) and assoc.n_rows == P
    ei = g[asc.LAB_EDGE].edge_index.numpy()
    assert np.array_equal(assoc.count, np.bincount(ei[1], minlength=L)) and int(assoc.count.sum()) == ei.shape[1]
    assert np.array_equal(np.diagonal(assoc.n), assoc.count) and np.array_equal(assoc.n, assoc.n.T)
    for f in ("lab_comeasurement.csv", "lab_correlation.csv", "lab_association_pairs.csv", "lab_coverage.csv"):
        assert (tmp_path / f).exists(), f
    assert sorted(os.listdir(tmp_path)) == sorted(["lab_comeasurement.csv", "lab_correlation.csv",
                                                   "lab_association_pairs.csv", "lab_coverage.csv"])
    co = pd.read_csv(tmp_path / "lab_comeasurement.csv", index_col=0)
    assert co.shape == (L, L) and np.array_equal(co.to_numpy(), assoc.n) and list(co.index) == list(co.columns)
    cr = pd.read_csv(tmp_path / "lab_correlation.csv", index_col=0)
    assert np.allclose(cr.to_numpy(), assoc.r, rtol=1e-12, atol=1e-15, equal_nan=True)
    pairs = pd.read_csv(tmp_path / "lab_association_pairs.csv")
    assert list(pairs.columns) == asc.PAIR_COLUMNS and len(pairs) == len(frames["pairs"]) > 0
    assert (pairs.n >= 30).all() and len(pairs) == int((np.triu(assoc.n, 1) >= 30).sum())
    key = np.where(pairs.r.isna(), -1.0, pairs.r.abs())
    assert (np.diff(key) <= 0).all()
    ok = pairs.r.notna()
    assert ((pairs.r_lower[ok] <= pairs.r[ok]) & (pairs.r[ok] <= pairs.r_upper[ok])).all()
    cov = pd.read_csv(tmp_path / "lab_coverage.csv")
    assert list(cov.columns) == asc.COVERAGE_COLUMNS == ["lab", "patients", "coverage", "mean", "std"] and len(cov) == L
    assert np.array_equal(cov.patients.to_numpy(), assoc.count) and np.allclose(cov.coverage, assoc.count / P)
    X = asc.lab_matrix(ei[0], ei[1], g[asc.LAB_EDGE].edge_attr.reshape(-1).numpy(), P, L)
    frame = pd.DataFrame(X.astype(np.float64))
    assert np.allclose(cov["mean"], frame.mean().to_numpy(), rtol=1e-12, equal_nan=True)
    assert np.allclose(cov["std"], frame.std().to_numpy(), rtol=1e-10, equal_nan=True)
    want = frame.corr(min_periods=30).to_numpy()
    assert nan_equal(assoc.r, want) and np.allclose(assoc.r, want, rtol=0, atol=1e-12, equal_nan=True)
    # without an output directory nothing is written and the frames are the same
    _, again = asc.lab_association(g, min_periods=30)
    assert again["pairs"].equals(frames["pairs"])
