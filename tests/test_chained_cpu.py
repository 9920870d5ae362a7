"""Chained-equations lab imputation without a GPU: the numpy restatement of mmgnn/chained.py against
sklearn.impute.IterativeImputer(Ridge(alpha), skip_complete=False) with sklearn's own distance from the 80-bit chain of
tests/chain_ref.py as the yardstick; the special cases against that loop reference; the stopping rule, the clips,
transform and the state; every refusal; the binding of libmmgnn_chain.so from its header; the baseline plumbing on a
small synthetic graph through the numpy path."""
import ctypes
import functools
import os
import re
import warnings

import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import _lib, ops
from mmgnn import chained as ch
from mmgnn import evaluate as ev
from mmgnn.chained import ChainedLabImputer
from mmgnn.synth import make_graph
from mmgnn.train import EdgeMasker
import chain_ref as ref

F32 = np.float32
ROUNDS = 5


def sklearn_imputer(alpha, max_iter, tol, order, **kw):
    from sklearn.experimental import enable_iterative_imputer  # noqa: F401
    from sklearn.impute import IterativeImputer
    from sklearn.linear_model import Ridge
    return IterativeImputer(Ridge(alpha=alpha), max_iter=max_iter, tol=tol, imputation_order=order, skip_complete=False,
                            **kw)


def sk_fit_transform(imp, X):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")              # "early stopping criterion not reached": tol = 0 never stops
        return imp.fit_transform(np.asarray(X, np.float64))


def dist(a, b):
    return float(np.nanmax(np.abs(np.asarray(a, ref.LD) - b), initial=0.0))


# ---------------------------------------------------------------------------------- the restatement against sklearn
@pytest.mark.parametrize("alpha", [1.0, 10.0])
@pytest.mark.parametrize("order", ["ascending", "roman"])
@pytest.mark.parametrize("n, L", [(70, 5), (300, 17), (400, 8), (1000, 50)])
def test_restatement_against_sklearn(n, L, order, alpha):
    """The restatement is at most 8 x as far from the 80-bit chain as sklearn's own IterativeImputer is (the factor
    association and preprocess use for two float64 evaluations that differ in summation order); visit order, n_iter_
    and the NaN pattern EQUAL."""
    X = ref.make_matrix(n, L, seed=n + L, density=0.6)
    assert np.isfinite(X).any(0).all(), "no shape has an empty lab"
    imp = ChainedLabImputer(alpha=alpha, max_iter=ROUNDS, tol=0, imputation_order=order).fit_matrix(X)
    sk = sklearn_imputer(alpha, ROUNDS, 0, order)
    S = sk_fit_transform(sk, X)
    want, labs, hist = ref.chain(X, alpha, ROUNDS, order)
    d_me, d_sk = dist(imp.imputed64_, want), dist(S, want)
    print(f"({n}, {L}) {order} alpha {alpha}: restatement {d_me:.2e}, sklearn {d_sk:.2e} from the 80-bit chain")
    assert d_sk > 0 and d_me <= 8 * d_sk
    assert [t.feat_idx for t in sk.imputation_sequence_[:L]] == labs == imp._state["order"].tolist()
    assert imp.n_iter_ == sk.n_iter_ == ROUNDS == len(imp.history_)
    out = imp.impute_matrix()
    assert out.dtype == F32 and not np.isnan(out).any() and not np.isnan(S).any()
    obs = np.isfinite(X)
    assert np.array_equal(out[obs].view(np.int32), X[obs].view(np.int32)), "observed cells pass through bit for bit"
    assert np.array_equal(out, imp.imputed64_.astype(F32)), "one rounding at the end"
    assert np.allclose(imp.history_, hist, rtol=1e-9, atol=0)


# ---------------------------------------------------------------------------------- special cases
def special_matrix(empty_patient):
    """(60, 9): lab 1 nobody has, lab 2 everybody has, lab 3 has one value, labs 5 and 6 are identical (values and
    mask), lab 7 is constant; with empty_patient, patient 4 has no lab at all (and lab 2 everybody else)."""
    X = ref.make_matrix(60, 9, seed=5, density=0.55)
    X[:, 1] = np.nan
    X[:, 2] = np.random.default_rng(1).standard_normal(60).astype(F32)
    X[:, 3] = np.nan
    X[17, 3] = F32(2.25)
    X[:, 6] = X[:, 5]
    X[~np.isnan(X[:, 7]), 7] = F32(-1.5)
    if empty_patient:
        X[4, :] = np.nan
    return X


@pytest.mark.parametrize("empty_patient", [False, True])
@pytest.mark.parametrize("order", ch.ORDERS)
def test_special_cases_against_the_loop_reference(order, empty_patient):
    """The yardstick is again sklearn's distance from the 80-bit chain, on the matrix without the lab nobody has (sklearn
    drops that column; here it stays NaN and takes no part), and never less than 8 ulp of the largest value: the float64
    roundings of a mean, of mu and of the result itself, half an ulp each, are in any float64 evaluation."""
    X = special_matrix(empty_patient)
    keep = [a for a in range(X.shape[1]) if a != 1]
    imp = ChainedLabImputer(alpha=1.0, max_iter=ROUNDS, tol=0, imputation_order=order).fit_matrix(X)
    want, labs, _ = ref.chain(X, 1.0, ROUNDS, order)
    assert imp._state["order"].tolist() == labs and 1 not in labs and set(labs) == set(keep)
    out, W = imp.impute_matrix(), imp.imputed64_
    assert np.isnan(out[:, 1]).all() and np.isnan(want[:, 1]).all() and not np.isnan(out[:, keep]).any()
    S = sk_fit_transform(sklearn_imputer(1.0, ROUNDS, 0, order), X[:, keep])
    d_me, d_sk = dist(W[:, keep], want[:, keep]), dist(S, want[:, keep])
    floor = 8 * ref.U * float(np.nanmax(np.abs(X)))
    print(f"special, {order}: restatement {d_me:.2e}, sklearn {d_sk:.2e}, floor {floor:.2e}")
    assert d_me <= max(8 * d_sk, floor)
    if empty_patient:
        assert np.isnan(X[4]).all() and not np.isnan(out[4, keep]).any()
    else:
        assert np.array_equal(out[:, 2], X[:, 2]), "a lab everybody has is passed through"
    assert np.all(W[np.arange(60) != 17, 3] == 2.25), "a lab with one value imputes that value"
    assert np.all(W[:, 7] == -1.5), "a constant lab imputes its constant"
    assert np.all(imp._state["coef"][:, 3, 0] == 0.0) and np.all(imp._state["coef"][:, 7, 0] == 0.0)
    assert np.array_equal(X[:, 5], X[:, 6], equal_nan=True) and np.isfinite(W[:, 5:7]).all()     # collinear: alpha decides
    assert np.array_equal(imp.transform(X), out, equal_nan=True)


def test_one_lab_imputes_its_mean():
    X = np.array([[1.0], [np.nan], [2.5], [np.nan], [4.0]], F32)
    imp = ChainedLabImputer(max_iter=3, tol=0).fit_matrix(X)
    want, labs, hist = ref.chain(X, 1.0, 3)
    assert labs == [0] and imp.n_iter_ == 3 and hist == [0.0, 0.0, 0.0]
    assert dist(imp.imputed64_, want) <= 8 * ref.U * 4.0
    assert np.array_equal(imp.impute_matrix(), np.array([[1.0], [2.5], [2.5], [2.5], [4.0]], F32))
    allnan = ChainedLabImputer(max_iter=2, tol=0).fit_matrix(np.full((3, 2), np.nan, F32))
    assert np.isnan(allnan.impute_matrix()).all() and allnan.history_ == [0.0, 0.0]


# ---------------------------------------------------------------------------------- the pieces
def test_host_moments_against_fsum():
    """Lattice inputs EQUAL the loop reference; generic ones sit inside (n_j + 8) 2^-53 x the absolute sum."""
    for lattice in (True, False):
        X = ref.make_matrix(300, 9, seed=3, density=0.5, lattice=lattice)
        center = assoc_center(X, lattice)
        W = ch.host_init(X, center)
        for j in (0, 4, 8):
            n_j, s, G = ch.host_moments(W, X, j, center)
            wn, ws, wG, sa, Ga = ref.moments(W, X, j, center)
            assert n_j == wn and np.array_equal(G, G.T)
            if lattice:
                assert np.array_equal(s, ws) and np.array_equal(G, wG)
            else:
                assert np.all(np.abs(s - ws) <= ref.moment_bound(n_j, sa))
                assert np.all(np.abs(G - wG) <= ref.moment_bound(n_j, Ga))


def assoc_center(X, lattice):
    from mmgnn.association import host_colstats
    import assoc_ref
    return assoc_ref.lattice_center(X.shape[1], 3) if lattice else host_colstats(X)[1]


def test_solve_satisfies_the_ridge_equations_and_counts_bad_pivots():
    X = ref.make_matrix(200, 7, seed=9, density=0.7)
    center = assoc_center(X, False)
    count = np.isfinite(X).sum(0)
    W = ch.host_init(X, center)
    n_j, s, G = ch.host_moments(W, X, 2, center)
    w, mu, bad = ch.host_solve(G, s, n_j, count, 2, 3.0)
    P = ch.predictors(count, 2)
    C = G - np.outer(s, s) / n_j
    A = C[np.ix_(P, P)] + 3.0 * np.eye(P.size)
    assert bad == 0 and w[2] == 0.0 and np.array_equal(mu, s / n_j)
    assert np.abs(A @ w[P] - C[P, 2]).max() <= 64 * ref.U * np.abs(A).sum(1).max() * np.abs(w).max()
    _, _, bad = ch.host_solve(-5.0 * np.eye(4), np.zeros(4), 10, np.full(4, 10), 0, 1.0)
    assert bad == 3, "three pivots of -5 + 1"


# ---------------------------------------------------------------------------------- stopping, clips, transform, state
@functools.lru_cache(maxsize=None)
def fitted(tol=0.0, order="ascending"):
    X = ref.make_matrix(400, 8, seed=408, density=0.6)
    return X, ChainedLabImputer(alpha=1.0, max_iter=10, tol=tol, imputation_order=order).fit_matrix(X)


def test_the_stopping_rule_is_sklearns():
    X, full = fitted()
    h = full.history_
    assert full.n_iter_ == 10 and len(h) == 10
    k = max(i for i in range(1, 10) if h[i] < min(h[:i]) / 1.5)      # the last round that undercuts all before it by a third
    top = float(np.nanmax(np.abs(X)))
    tol = float(np.sqrt(h[k] * min(h[:k]))) / top                     # the threshold between them
    assert k >= 2 and min(h[:k]) > 1.2 * tol * top and h[k] < tol * top / 1.2, "an asserted gap: rounding cannot cross it"
    imp = ChainedLabImputer(alpha=1.0, max_iter=10, tol=tol).fit_matrix(X)
    assert imp.n_iter_ == k + 1 and imp.history_ == h[:k + 1] and imp._state["coef"].shape == (k + 1, 8, 2, 8)
    sk = sklearn_imputer(1.0, 10, tol, "ascending")
    sk_fit_transform(sk, X)
    assert sk.n_iter_ == imp.n_iter_
    _, _, hist = ref.chain(X, 1.0, 10, tol=tol)
    assert len(hist) == imp.n_iter_


def test_clips_are_honoured_and_are_sklearns():
    X, free = fitted()
    L = X.shape[1]
    miss = ~np.isfinite(X)
    lo = np.nanpercentile(np.where(miss, free.imputed64_, np.nan), 30, axis=0)
    hi = np.nanpercentile(np.where(miss, free.imputed64_, np.nan), 70, axis=0)
    imp = ChainedLabImputer(max_iter=ROUNDS, tol=0, min_value=lo, max_value=hi).fit_matrix(X)
    W = imp.imputed64_
    assert np.all((W >= lo[None, :])[miss]) and np.all((W <= hi[None, :])[miss])
    assert (W == lo[None, :])[miss].any() and (W == hi[None, :])[miss].any() and ((W > lo) & (W < hi))[miss].any()
    obs = ~miss
    assert np.array_equal(imp.impute_matrix()[obs], X[obs]), "an observed cell is never clipped"
    want, _, _ = ref.chain(X, 1.0, ROUNDS, lo=lo, hi=hi)
    S = sk_fit_transform(sklearn_imputer(1.0, ROUNDS, 0, "ascending", min_value=lo, max_value=hi), X)
    d_me, d_sk = dist(W, want), dist(S, want)
    print(f"clipped: restatement {d_me:.2e}, sklearn {d_sk:.2e} from the 80-bit chain")
    assert d_me <= 8 * d_sk
    scalar = ChainedLabImputer(max_iter=2, tol=0, min_value=-0.25, max_value=0.5).fit_matrix(X)
    assert np.all(scalar.imputed64_[miss] >= -0.25) and np.all(scalar.imputed64_[miss] <= 0.5)


def test_transform_of_the_training_matrix_is_bitwise_the_fit_and_rows_are_independent():
    X, imp = fitted()
    out = imp.impute_matrix()
    again = imp.transform(X)
    assert again.dtype == F32 and np.array_equal(again.view(np.int32), out.view(np.int32))
    rows = np.array([5, 399, 0, 77])
    assert np.array_equal(imp.transform(X[rows]).view(np.int32), out[rows].view(np.int32))
    assert np.array_equal(imp.impute_matrix(rows), out[rows])
    assert np.array_equal(imp.predict(rows, np.array([0, 7, 3, 3])), out[rows, [0, 7, 3, 3]])
    t = imp.transform(torch.from_numpy(X[rows]))
    assert torch.is_tensor(t) and np.array_equal(t.numpy(), out[rows])
    assert np.array_equal(imp.transform(X, return_float64=True), imp.imputed64_)


def test_state_dict_round_trip():
    X, imp = fitted(0.0, "descending")
    state = imp.state_dict()
    assert all(torch.is_tensor(state[k]) for k in ("count", "center", "order", "coef", "lo", "hi"))
    assert state["coef"].shape == (10, 8, 2, 8) and state["coef"].dtype == torch.float64
    other = ChainedLabImputer().load_state_dict({k: (v.clone() if torch.is_tensor(v) else v) for k, v in state.items()})
    assert other.n_iter_ == 10 and other.history_ == imp.history_ and other.imputation_order == "descending"
    assert np.array_equal(other.transform(X).view(np.int32), imp.impute_matrix().view(np.int32))
    with pytest.raises(RuntimeError, match="transform"):
        other.impute_matrix()
    with pytest.raises(KeyError, match="coef"):
        ChainedLabImputer().load_state_dict({k: v for k, v in state.items() if k != "coef"})
    with pytest.raises(RuntimeError, match="fit"):
        ChainedLabImputer().transform(X)


# ---------------------------------------------------------------------------------- refusals
def test_every_refusal():
    X = ref.make_matrix(30, 4, seed=1)
    for kw, msg in ((dict(alpha=0.0), "alpha"), (dict(alpha=-1.0), "alpha"), (dict(alpha=float("nan")), "alpha"),
                    (dict(max_iter=0), "max_iter"), (dict(tol=-1e-3), "tol"), (dict(imputation_order="random"), "order"),
                    (dict(imputation_order="zigzag"), "order"), (dict(min_value=1.0, max_value=1.0), "min_value"),
                    (dict(min_value=np.zeros(3)), "min_value")):
        with pytest.raises(ValueError, match=msg):
            ChainedLabImputer(**kw).fit_matrix(X)
    with pytest.raises(ValueError, match="labs"):
        ChainedLabImputer().fit_matrix(np.zeros((4, 129), F32))
    with pytest.raises(ValueError, match="2-D"):
        ChainedLabImputer().fit_matrix(np.zeros(4, F32))
    bad = X.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="1 infinite"):
        ChainedLabImputer().fit_matrix(bad)
    p, lab, v = np.array([0, 0, 2]), np.array([0, 1, 1]), np.array([1.0, 2.0, 3.0], F32)
    for args, msg in (((p, lab, v, 3, 129), "n_labs"), ((p, lab, v, 0, 2), "n_patients"), ((p, lab, v, 2, 2), "patient index"),
                      ((p, lab, v, 3, 1), "lab index"), ((p, lab, v[:2], 3, 2), "one entry per cell"),
                      ((p.astype(np.float64), lab, v, 3, 2), "integers"),
                      ((p, lab, np.array([1, np.nan, 3], F32), 3, 2), "NaN"),
                      ((np.array([0, 0, 2]), np.array([1, 1, 1]), v, 3, 2), "duplicate")):
        with pytest.raises(ValueError, match=msg):
            ChainedLabImputer().fit(*args)
    imp = ChainedLabImputer(max_iter=2).fit(p, lab, v, 3, 2)
    assert isinstance(imp.impute_matrix(), np.ndarray) and imp.impute_matrix().shape == (3, 2)
    with pytest.raises(ValueError, match="labs"):
        imp.transform(np.zeros((2, 3), F32))
    with pytest.raises(ValueError, match="infinite"):
        imp.transform(np.array([[np.inf, 1.0]], F32))
    with pytest.raises(ValueError, match="patient index"):
        imp.predict(np.array([3]), np.array([0]))
    with pytest.raises(ValueError, match="lab index"):
        imp.predict(np.array([0]), np.array([2]))
    with pytest.raises(_lib.MmgError, match="device tensor"):               # never the host path behind the kernels' door
        from mmgnn import chain_ops
        chain_ops.chain_init(torch.zeros(4, 3), torch.zeros(3, dtype=torch.float64))


# ---------------------------------------------------------------------------------- the binding
def test_the_chain_header_parses_and_names_what_the_library_defines():
    from mmgnn import chain_ops as m
    b = m.BINDING
    assert isinstance(b, _lib.Binding) and b.stem == "chain"
    assert os.path.basename(b.lib_path) == "libmmgnn_chain.so" and os.path.basename(b.header_path) == "mmgnn_chain.h"
    assert (m.DEFINES, m.SIGNATURES, m.PARAMS) == (b.defines, b.signatures, b.params)
    text = re.sub(r"/\*.*?\*/", "", open(b.header_path).read(), flags=re.S)
    assert sorted(re.findall(r"^\s*#\s*define\s+(MMG_\w+)", text, flags=re.M)) == sorted(b.defines) and b.defines
    for name, v in b.defines.items():
        assert type(v) is int and getattr(m, name) == v
    assert m.CH_MAX_LABS == ch.MAX_LABS == 128
    assert not set(b.signatures) & set(_lib.SIGNATURES)
    assert os.path.exists(b.lib_path), f"{b.lib_path} is not built (make -C multi-modal-gnn_amd/csrc)"
    ctypes.CDLL(_lib.LIB_PATH, mode=ctypes.RTLD_GLOBAL)               # the satellite links against it
    raw = ctypes.CDLL(b.lib_path)
    for sym in b.signatures:
        assert hasattr(raw, sym), sym
    assert sorted(b.signatures) == sorted(
        f"mmg_chain_{s}" for s in ("plan", "init", "moments", "moments_ws_bytes", "solve", "apply", "apply_ws_bytes",
                                   "finish"))
    with_ws = [sym for sym, params in b.params.items() if any(p[0] == "ws" for p in params)]
    assert sorted(with_ws) == ["mmg_chain_apply", "mmg_chain_moments"]
    for sym in with_ws:
        assert sym + "_ws_bytes" in b.signatures and b.signatures[sym + "_ws_bytes"][0] is ctypes.c_size_t, sym
        assert [p[0] for p in b.params[sym]][-3:] == ["ws", "ws_bytes", "stream"], sym
        assert b.params[sym][-3][1:] == ("void", 1) and b.params[sym][-2][1:] == ("size_t", 0), sym
    for sym, params in b.params.items():
        if not sym.endswith(("_plan", "_ws_bytes")):
            assert params[-1][0] == "stream", sym
    assert sorted(ops._plans(b)) == sorted(b.signatures)


def test_the_plan_and_the_host_refusals_of_the_library():
    """mmg_chain_plan and every argument check run on the host: no device is needed (null device pointers are refused
    after the shape)."""
    from mmgnn import chain_ops as m
    lib = m.load()
    for n, L in ((1, 1), (255, 50), (256, 50), (257, 50), (183400, 50), (183400, 128), (2 ** 31 - 2, 128), (5000, 65)):
        rows, slabs = m.chain_plan(n, L)
        nb = (L + m.CH_TILE - 1) // m.CH_TILE
        target = m.MMG_CH_BLOCKS // (nb * (nb + 1) // 2)
        want = max(m.MMG_CH_MIN_ROWS, -(-(-(-n // target)) // m.CH_CHUNK) * m.CH_CHUNK)
        assert rows == want and rows % m.CH_CHUNK == 0 and slabs == -(-n // rows)
        assert lib.mmg_chain_moments_ws_bytes(n, L) >= slabs * (L * L + L + 1) * 8
        assert lib.mmg_chain_apply_ws_bytes(n, L) >= -(-n // m.CH_APPLY_ROWS) * 8
    for n, L in ((0, 5), (2 ** 31 - 1, 5), (10, 0), (10, 129)):
        assert lib.mmg_chain_moments_ws_bytes(n, L) == 0 and lib.mmg_chain_apply_ws_bytes(n, L) == 0
        with pytest.raises(_lib.MmgError, match="chain_plan"):
            m.chain_plan(n, L)
    E_ARG, E_WS = _lib.MMG_E_ARG, _lib.MMG_E_WS
    assert lib.mmg_chain_moments(None, None, 10, 129, 200, 0, None, None, None, None, None, 0, None) == E_ARG
    assert lib.mmg_chain_moments(None, None, 10, 8, 7, 0, None, None, None, None, None, 0, None) == E_ARG
    assert b"ld_x 7 < L 8" in _lib.load().mmg_last_error()
    assert lib.mmg_chain_moments(None, None, 10, 8, 8, 8, None, None, None, None, None, 0, None) == E_ARG
    assert b"target 8" in _lib.load().mmg_last_error()
    assert lib.mmg_chain_moments(None, None, 10, 8, 8, 0, None, None, None, None, None, 0, None) == E_ARG   # null pointers
    assert lib.mmg_chain_init(None, 0, 8, 8, None, None, None) == E_ARG
    assert lib.mmg_chain_solve(None, None, None, None, 8, 0, 0.0, None, None, None, None) == E_ARG
    assert b"alpha" in _lib.load().mmg_last_error()
    assert lib.mmg_chain_solve(None, None, None, None, 8, -1, 1.0, None, None, None, None) == E_ARG
    assert lib.mmg_chain_solve(None, None, None, None, 8, 0, float("inf"), None, None, None, None) == E_ARG
    assert lib.mmg_chain_apply(None, None, 10, 8, 8, 9, None, None, None, None, None, None, 0, None, None, 0, None) == E_ARG
    assert lib.mmg_chain_finish(None, None, 10, 8, 8, None, None, 7, None) == E_ARG
    assert b"ld_out" in _lib.load().mmg_last_error()
    assert E_ARG != E_WS


# ---------------------------------------------------------------------------------- the drivers
def test_the_baseline_plumbing_on_a_synthetic_graph_through_the_numpy_path():
    g = make_graph(1, seed=0)
    masker = EdgeMasker(g)
    P, L = int(g["patient"].num_nodes), int(g["lab"].num_nodes)
    assert "chained_equations" in ev.BASELINES
    tr_ei, tr_v, _, _ = masker.get_masked_data("train", want_mask=False)
    te_ei, te_v, _, _ = masker.get_masked_data("test", want_mask=False)
    fitted_ = ev.fit_baselines(("per_lab_mean", "chained_equations"), tr_ei, tr_v.reshape(-1), L, P)
    kind, (imp, g_mean) = fitted_["chained_equations"]
    assert kind == "chained_equations" and isinstance(imp, ChainedLabImputer) and 1 <= imp.n_iter_ <= 10
    pairs = ev.baseline_pairs(fitted_["chained_equations"], te_ei[0], te_ei[1])
    assert torch.is_tensor(pairs) and pairs.dtype == torch.float32 and pairs.shape == (te_ei.shape[1],)
    assert bool(torch.isfinite(pairs).all())
    rows = torch.tensor([0, 5, P - 1])
    dense = ev.baseline_matrix(fitted_["chained_equations"], rows, L)
    assert dense.shape == (3, L) and bool(torch.isfinite(dense).all())
    X = imp.impute_matrix()
    assert torch.equal(dense, torch.where(torch.isnan(X[rows]), g_mean, X[rows]))
    assert torch.equal(pairs, dense.new_tensor(X[te_ei[0], te_ei[1]].numpy()))
    tr = tr_ei.numpy()
    assert np.array_equal(X[tr[0], tr[1]].numpy(), tr_v.reshape(-1).numpy()), "train values pass through"
    res = ev.evaluate_chained_baseline(g, masker, "test", max_iter=3, tol=0.0)
    assert list(res) == ["chained_equations"]
    want = ev.compute_regression_metrics(ChainedLabImputer(max_iter=3, tol=0.0).fit(
        tr[0], tr[1], tr_v.reshape(-1).numpy(), P, L).predict(te_ei[0].numpy(), te_ei[1].numpy()), te_v.reshape(-1).numpy())
    assert res["chained_equations"] == want and set(want) >= {"mae", "rmse", "r2"}
    print(f"synthetic x1, test split: chained_equations MAE {want['mae']:.4f}")
    with pytest.raises(ValueError, match="unknown baseline"):
        ev.fit_baselines(("median",), tr_ei, tr_v.reshape(-1), L, P)
