"""Stacked recalibration on the host (mmgnn/stacking.py): the numpy restatement against the loop reference of
stack_ref.py -- sums within the documented order's error bound of the exact ones and EQUAL on lattice inputs, the
coefficients against an 80-bit solve with numpy.linalg.solve's own distance as the yardstick, every fallback level,
the folds, that it helps on data built for it -- and the plumbing around it (state dict, inference dicts, the derived
binding)."""
import inspect
import json
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import inference
from mmgnn import stacking as st
import stack_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
EDGES3 = [0.0, 6.0, 16.0, float("inf")]
EDGES1 = [1.0, 6.0, 16.0, float("inf")]                      # degree 0 lies in no bin


def same(a, b):
    """equal as values: the same NaN positions, the same infinities, equal numbers (-0 == +0)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def host_sums(c, edges, folds=1, seed=0):
    return st.host_sums(c["feats"], c["target"], c["patient"], c["lab"], c["n_labs"], c["deg"], edges, folds, seed)


# ---------------------------------------------------------------------------------- sums
@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("folds", [1, 3])
def test_sums_lie_within_the_order_bound_of_the_exact_sums(K, folds):
    """A term goes through at most 16 (slot) + 6 (butterfly) + 4 (waves) + n_chunks additions: |sum - exact| <=
    (28 + n_chunks) 2^-53 sum |terms| (+ the one rounding of the exact sum)."""
    c = ref.make_case(seed=K, n=10000, K=K, n_labs=2, n_pat=40)
    c["feats"][0][12], c["target"][13] = F32(2.5), F32(-1.5)        # (finite values: the bound is about rounding)
    edges = [1.0, float("inf")]                                      # degree 0 lies in no bin
    got, dropped = host_sums(c, edges, folds, 5)
    want, mags, rdrop = ref.fsum_sums(c, edges, folds, 5)
    assert got.shape == want.shape == (folds, 2, st.n_fields(K)) and same(dropped, rdrop)
    assert dropped.tolist()[:2] == [5, 2] and dropped[2] > 0 and dropped[3] == 3
    assert same(got[:, :, 0], want[:, :, 0])                        # the counts are exact
    n_chunks = np.ceil(want[:, :, :1] / st.ST_CHUNK)
    bound = (29 + n_chunks) * 2.0 ** -53 * mags
    assert (np.abs(got - want) <= bound).all()
    # a cell of two chunks (one fold) / of several pairs per slot (three folds); and the orders do differ
    assert want[:, :, 0].max() > (st.ST_CHUNK if folds == 1 else 1024) and np.abs(got - want).max() > 0


@pytest.mark.parametrize("K", [1, 4])
def test_sums_are_exact_on_lattice_inputs(K):
    c = ref.make_case(seed=3, n=9000, K=K, n_labs=1, n_pat=40, lattice=True)
    for folds in (2, 1):
        got, dropped = host_sums(c, [0.0, float("inf")], folds, 1)
        want, _, rdrop = ref.fsum_sums(c, [0.0, float("inf")], folds, 1)
        assert same(got, want) and same(dropped, rdrop)
    assert want[0, 0, 0] > 2 * st.ST_CHUNK                           # a cell of three chunks


# ---------------------------------------------------------------------------------- solve
def test_coefficients_against_the_80_bit_solve():
    """Distance to the 80-bit solution of the same float64 systems, over all usable systems of K = 1 .. 4, ridge 0 and
    1e-3: the restatement's Cholesky may be at most 8x as far from it as numpy.linalg.solve is.
    Measured (max |w - w80| over the systems, restatement vs numpy.linalg.solve): K=1 3.29e-16 vs 1.77e-16 (ratio
    1.86), K=2 3.70e-16 vs 1.87e-16 (1.98), K=3 3.36e-16 vs 2.84e-16 (1.18), K=4 9.12e-16 vs 9.58e-16 (0.95)."""
    assert np.finfo(np.longdouble).nmant >= 63, "no 80-bit long double on this platform"
    for K in (1, 2, 3, 4):
        c = ref.make_case(seed=10 + K, n=4000, K=K, n_labs=4, n_pat=40)
        c["feats"][0][12], c["target"][13] = F32(2.5), F32(-1.5)
        d_mine = d_np = 0.0
        for ridge in (0.0, 1e-3):
            sums, _ = host_sums(c, EDGES3, 3, 2)
            coef, level, n_used = st.host_solve(sums, 4, 3, K, ridge, 30)
            rcoef, rlevel, rused, taken = ref.solve(sums, 4, 3, K, ridge, 30)
            assert same(level, rlevel) and same(n_used, rused) and len(taken) == level.size
            w80 = np.stack([ref.solve_ld(A, r) for A, r in taken]).reshape(coef.shape)
            d_mine = max(d_mine, float(np.abs(coef - w80).max()))
            d_np = max(d_np, float(np.abs(rcoef - w80).max()))
        print(f"K={K}: restatement {d_mine:.2e}, numpy.linalg.solve {d_np:.2e}, ratio {d_mine / d_np:.2f}")
        assert d_mine <= 8 * d_np


def test_fallback_levels_one_by_one():
    rng = np.random.default_rng(2)
    n_labs, n_pat = 3, 30
    deg = np.array([3] * 10 + [9] * 10 + [20] * 10, np.int32)                # bins 0, 1, 2
    rows = []
    for lab in range(n_labs):
        for b in range(3):
            m = 200
            if (lab, b) == (0, 1):
                m = 12                                                          # below min_count: falls back to the lab
            for _ in range(m):
                rows.append((lab, b * 10 + rng.integers(0, 10)))
    lab, patient = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    t = rng.standard_normal(lab.size).astype(F32)
    f1 = (0.5 * t + 0.5 * rng.standard_normal(lab.size)).astype(F32)
    f2 = rng.standard_normal(lab.size).astype(F32)
    twin = (lab == 1) & (deg[patient] == 20)
    f2[twin] = f1[twin]                                                         # two identical features: singular at the cell
    c = dict(feats=[f1, f2], target=t, patient=patient, lab=lab, n_labs=n_labs, deg=deg)
    sums, _ = host_sums(c, EDGES3)
    coef, level, n_used = st.host_solve(sums, n_labs, 3, 2, 0.0, 30)
    rcoef, rlevel, rused, _ = ref.solve(sums, n_labs, 3, 2, 0.0, 30)
    assert same(level, rlevel) and same(n_used, rused) and np.allclose(coef, rcoef, rtol=1e-9, atol=1e-12)
    want = np.zeros((1, 9), np.int32)
    want[0, 1], want[0, 5] = 1, 1
    assert same(level, want)
    assert n_used[0, 1] == 412 and n_used[0, 5] == 600 and n_used[0, 0] == 200
    # the lab level of lab 0 is the regression over its three cells' pairs
    sel = lab == 0
    X = np.stack([np.ones(sel.sum()), f1[sel].astype(np.float64), f2[sel].astype(np.float64)], axis=1)
    w = np.linalg.lstsq(X, t[sel].astype(np.float64), rcond=None)[0]
    assert np.allclose(coef[0, 1], w, rtol=1e-9, atol=1e-12)
    # ridge = 0 against lstsq in every cell fitted at its own level
    for cell in (0, 2, 3, 4, 6, 7, 8):
        sel = (lab == cell // 3) & (np.searchsorted([6, 16], deg[patient], "right") == cell % 3)
        X = np.stack([np.ones(sel.sum()), f1[sel].astype(np.float64), f2[sel].astype(np.float64)], axis=1)
        w = np.linalg.lstsq(X, t[sel].astype(np.float64), rcond=None)[0]
        assert np.allclose(coef[0, cell], w, rtol=1e-9, atol=1e-12), cell
    # everything unusable: e, level 3, and the prediction is f_1
    coef, level, n_used = st.host_solve(sums, n_labs, 3, 2, 1e-3, 10 ** 6)
    assert set(level.reshape(-1).tolist()) == {3} and not n_used.any()
    assert same(coef, np.broadcast_to(np.array([0.0, 1.0, 0.0]), coef.shape))
    assert same(st.host_apply_pairs([f1, f2], patient, lab, n_labs, deg, EDGES3, coef), f1)
    # all three features identical and no ridge: singular at every level
    c2 = dict(c, feats=[f1, f1])
    s2, _ = host_sums(c2, EDGES3)
    assert set(st.host_solve(s2, n_labs, 3, 2, 0.0, 0)[1].reshape(-1).tolist()) == {3}
    assert set(ref.solve(s2, n_labs, 3, 2, 0.0, 0)[1].reshape(-1).tolist()) == {3}
    # the cell level gone, the lab level gone, all pairs left
    coef, level, n_used = st.host_solve(sums, n_labs, 3, 2, 1e-3, 700)
    assert set(level.reshape(-1).tolist()) == {2} and set(n_used.reshape(-1).tolist()) == {lab.size}


def test_apply_equals_the_loop_reference():
    c = ref.make_case(seed=4, n=3000, K=3)
    sums, _ = host_sums(c, EDGES1, 4, 9)
    coef, _, _ = st.host_solve(sums, 5, 3, 3, 1e-3, 30)
    for cross in (False, True):
        got = st.host_apply_pairs(c["feats"], c["patient"], c["lab"], 5, c["deg"], EDGES1, coef, 9, cross)
        assert same(got, ref.apply_pairs(c, EDGES1, coef, 9, cross))
    assert np.isnan(got[10]) and np.isnan(got[11]) and not np.isnan(got[9])   # a NaN feature gives NaN; the target is no input
    assert np.isnan(got[0]) and got[7] == c["feats"][0][7]           # no cell: f_1 as it is (here NaN / the value)
    sc, dropped = st.host_scores(c["feats"][0], got, c["target"], c["patient"], c["lab"], 5, c["deg"], EDGES1)
    assert sc.shape == (15 + 5 + 1, 5) and sc[-1, 0] + dropped.sum() == 3000
    assert same(sc[15:20, 0], sc[:15, 0].reshape(5, 3).sum(1)) and sc[-1, 0] == sc[15:20, 0].sum()


# ---------------------------------------------------------------------------------- folds
def test_folds_are_a_function_of_the_patient_and_fold_out_sums_leave_the_fold_out():
    c = ref.make_case(seed=6, n=4000, K=2, special=False)
    for folds in (2, 5, 8):
        f = st.host_folds(c["patient"], folds, 11)
        assert [int(v) for v in f[:200]] == [ref.fold_of(p, folds, 11) for p in c["patient"][:200]]
        assert set(f.tolist()) == set(range(folds))
        for p in np.unique(c["patient"]):
            assert len(set(f[c["patient"] == p].tolist())) == 1
        assert not same(f, st.host_folds(c["patient"], folds, 12))  # the seed moves the folds
        sums, _ = host_sums(c, EDGES3, folds, 11)
        T = st.host_training_sums(sums)
        assert T.shape[0] == folds + 1
        for j in range(folds):
            rest = dict(c, feats=[x[f != j] for x in c["feats"]], target=c["target"][f != j], patient=c["patient"][f != j],
                        lab=c["lab"][f != j])
            want, _, _ = ref.fsum_sums(rest, EDGES3)
            assert same(T[j][:, 0], want[0][:, 0])                  # exactly the pairs of the other folds
            assert np.allclose(T[j], want[0], rtol=1e-12, atol=1e-12)
        assert same(T[folds][:, 0], ref.fsum_sums(c, EDGES3)[0][0][:, 0])
    s = st.LabStacker(folds=1).fit(c["feats"], c["target"], c["lab"], c["patient"], c["deg"], n_labs=5)
    with pytest.raises(ValueError):
        s.cross_fit_predict(c["feats"], c["lab"], c["patient"])
    s5 = st.LabStacker(folds=5, seed=3).fit(c["feats"], c["target"], c["lab"], c["patient"], c["deg"], n_labs=5)
    oof, ins = s5.cross_fit_predict(c["feats"], c["lab"], c["patient"]), s5.predict(c["feats"], c["lab"], c["patient"])
    assert not same(oof, ins)
    assert np.allclose(s5.coef[-1], s.coef[-1], rtol=1e-9, atol=1e-12)           # all folds together: all pairs


# ---------------------------------------------------------------------------------- it helps
def test_stacking_helps_on_a_flat_offset_predictor():
    fit, ev = ref.flat_gnn_split()
    # the loop reference alone, first
    sums, _, _ = ref.fsum_sums(fit, EDGES3)
    rcoef, _, _, _ = ref.solve(sums, 10, 3, 2, 1e-3, 30)
    ry = ref.apply_pairs(ev, EDGES3, rcoef)

    def mse(y, sel=slice(None)):
        return float(np.mean((ev["target"][sel].astype(np.float64) - y[sel].astype(np.float64)) ** 2))

    raw = ev["feats"][0]
    labs_better = sum(mse(ry, ev["lab"] == l) < mse(raw, ev["lab"] == l) for l in range(10))
    assert mse(ry) < mse(raw) and labs_better >= 9, "the loop reference itself does not help on this seed"
    s = st.LabStacker().fit(fit["feats"], fit["target"], fit["lab"], fit["patient"], fit["deg"], n_labs=10)
    y = s.predict(ev["feats"], ev["lab"], ev["patient"])
    labs_better = sum(mse(y, ev["lab"] == l) < mse(raw, ev["lab"] == l) for l in range(10))
    print(f"MSE raw {mse(raw):.4f} -> stacked {mse(y):.4f}; better in {labs_better} of 10 labs")
    assert mse(y) < mse(raw) and labs_better >= 9
    frame = s.scores(ev["feats"], ev["target"], ev["lab"], ev["patient"])
    assert list(frame.columns) == st.SCORE_COLUMNS and len(frame) == 1 + 10 + 30
    top = frame.iloc[0]
    assert top["n"] == ev["target"].size and np.isclose(top["rmse_stacked"] ** 2, mse(y)) and np.isclose(top["rmse_raw"] ** 2, mse(raw))
    assert top["mae_stacked"] < top["mae_raw"]


# ---------------------------------------------------------------------------------- plumbing
def test_state_dict_round_trip_and_table_frame():
    c = ref.make_case(seed=8, n=2500, K=2)
    a = st.LabStacker(ridge=1e-2, min_count=20, folds=3, seed=4)
    a.fit({"gnn": c["feats"][0], "per_lab_mean": c["feats"][1]}, c["target"], c["lab"], c["patient"], c["deg"], n_labs=5)
    state = a.state_dict()
    assert all(isinstance(v, (np.ndarray, int, float, str, list)) for v in state.values())
    b = st.LabStacker().load_state_dict(state)
    assert (b.ridge, b.min_count, b.folds, b.seed, b.n_labs, b.n_features, b.edges, b.labels, b.feature_names) == \
        (a.ridge, a.min_count, a.folds, a.seed, a.n_labs, a.n_features, a.edges, a.labels, a.feature_names)
    for x, y in zip(a._host, b._host):
        assert same(x, y)
    for fn in ("predict", "cross_fit_predict"):
        assert same(getattr(a, fn)(c["feats"], c["lab"], c["patient"]), getattr(b, fn)(c["feats"], c["lab"], c["patient"]))
    m = c["feats"][0][:20].reshape(4, 5).copy()
    m[0, 0] = 0.25                                                   # (the case's NaN)
    vec = np.arange(5, dtype=F32) / 4
    rows = np.array([3, 3, 0, 39])
    pm = a.predict_matrix([m, vec], rows)
    pp = a.predict([m.reshape(-1), np.tile(vec, 4)], np.tile(np.arange(5), 4), rows.repeat(5))
    assert same(pm.reshape(-1), pp) and not same(pm, m)
    frame = a.table_frame({0: "glucose"})
    assert list(frame.columns) == ["lab_idx", "lab_name", "degree_bin", "n_used", "level", "intercept", "w_gnn", "w_per_lab_mean"]
    assert len(frame) == 15 and frame.lab_name[0] == "glucose" and frame.degree_bin.tolist()[:3] == ["0-5", "6-15", "16+"]
    assert set(frame.level) <= set(st.LEVELS)
    for bad in (dict(ridge=-1.0), dict(ridge=float("nan")), dict(folds=0), dict(folds=9), dict(min_count=-1)):
        with pytest.raises(ValueError):
            st.LabStacker(**bad)
    with pytest.raises(RuntimeError):
        st.LabStacker().predict(c["feats"], c["lab"], c["patient"])
    with pytest.raises(ValueError):
        a.predict(c["feats"][:1], c["lab"], c["patient"])           # fitted on two predictors
    with pytest.raises(ValueError):
        st.LabStacker().fit([c["feats"][0]] * 5, c["target"], c["lab"], c["patient"], c["deg"], n_labs=5)


class FakeModel:
    """impute_lab_matrix without a device: a fixed function of (patient, lab)."""

    def impute_lab_matrix(self, data, rows):
        labs = torch.arange(int(data["lab"].num_nodes), dtype=torch.float32)
        return torch.sin(rows.to(torch.float32)[:, None] * 0.37 + labs[None, :] * 1.3) * 0.75


def inference_case():
    from mmgnn.synth import make_graph
    from mmgnn.train import EdgeMasker
    g = make_graph(1, seed=0)
    lab_indexer = {f"L{i}": i for i in range(50)}
    lab_stats = pd.DataFrame({"ITEMID": list(lab_indexer), "mean": np.linspace(1.0, 2.0, 50), "std": np.linspace(0.5, 1.5, 50)})
    pidx = {str(i): i for i in range(int(g["patient"].num_nodes))}
    return g, ([5, 1833, 7], g, FakeModel(), torch.device("cpu"), None, lab_stats, EdgeMasker(g), pidx, lab_indexer)


def test_inference_default_path_is_what_it_was_and_a_stacker_adds_the_raw_prediction():
    """tests/golden/stack_inference_default.json holds the dicts predict_for_patients returned for inference_case()
    BEFORE the stacker keywords existed (recorded with the module of that commit): the default path gives them still."""
    g, args = inference_case()
    with open(os.path.join(REPO, "tests", "golden", "stack_inference_default.json")) as f:
        golden = json.load(f)
    plain = inference.predict_for_patients(*args)
    assert plain == golden
    assert inference.predict_for_patient(1833, *args[1:]) == golden[1]
    assert sum(len(d["masked_labs"]) for d in golden) > 0 and sum(len(d["truly_missing_labs"]) for d in golden) > 0
    for fn in (inference.predict_for_patients, inference.predict_for_patient):
        assert inspect.signature(fn).parameters["stacker"].default is None
        assert inspect.signature(fn).parameters["stack_features"].default is None
    # a stacker: fitted on the host on (fake prediction, per-lab vector) of the graph's own edges
    ei = g["patient", "has_lab", "lab"].edge_index.numpy()
    y = g["patient", "has_lab", "lab"].edge_attr.reshape(-1).numpy().astype(F32)
    pred = FakeModel().impute_lab_matrix(g, torch.arange(1834)).numpy()
    vec = torch.linspace(-0.5, 0.5, 50)
    s = st.LabStacker().fit([pred[ei[0], ei[1]], vec.numpy()[ei[1]]], y, ei[1], ei[0], g, n_labs=50)
    stacked = inference.predict_for_patients(*args, stacker=s, stack_features=[vec])
    want = s.predict_matrix([pred[[5, 1833, 7]], vec.numpy()], np.array([5, 1833, 7]))
    stats = args[5]
    for row, a_, b_ in zip(range(3), plain, stacked):
        assert a_["measured_labs"] == b_["measured_labs"]
        for group in ("masked_labs", "truly_missing_labs"):
            assert list(a_[group]) == list(b_[group])
            for name, entry in b_[group].items():
                base, li = a_[group][name], args[8][name]
                assert set(entry) == set(base) | {"raw_prediction", "normalized_raw_prediction"}
                assert entry["raw_prediction"] == base["predicted"]
                assert entry["normalized_raw_prediction"] == base["normalized_predicted"]
                assert entry["normalized_predicted"] == float(want[row, li])
                assert entry["predicted"] == float(want[row, li] * stats.iloc[li]["std"] + stats.iloc[li]["mean"])


def test_binding_is_derived_from_the_header_and_matches_the_library():
    from mmgnn import stack_ops as so
    from mmgnn import conformal_ops as co
    calls = {"mmg_stack_sums", "mmg_stack_solve", "mmg_stack_apply_pairs", "mmg_stack_apply_matrix", "mmg_stack_scores"}
    with_ws = calls - {"mmg_stack_apply_pairs", "mmg_stack_apply_matrix"}
    assert set(so.SIGNATURES) == calls | {c + "_ws_bytes" for c in with_ws}
    for name in with_ws:
        assert [p[0] for p in so.PARAMS[name]][-3:] == ["ws", "ws_bytes", "stream"], name
    for name in calls - with_ws:
        assert [p[0] for p in so.PARAMS[name]][-1] == "stream" and "ws" not in [p[0] for p in so.PARAMS[name]]
    assert (so.ST_MAX_FEATURES, so.ST_MAX_FOLDS, so.ST_CHUNK, so.ST_DROP_KINDS, so.ST_SCORE_FIELDS) == (4, 8, 4096, 4, 5)
    assert (so.ST_MAX_LABS, so.ST_MAX_BINS, so.ST_MAX_CELLS) == (co.CF_MAX_LABS, co.CF_MAX_BINS, co.CF_MAX_CELLS)
    assert (so.ST_SITE, so.ST_CHUNK, so.ST_PIVOT_REL) == (st.ST_SITE, st.ST_CHUNK, st.PIVOT_REL) and so.ST_SITE == ref.ST_SITE
    assert (so.ST_MAX_FEATURES, so.ST_MAX_FOLDS) == (st.ST_MAX_FEATURES, st.ST_MAX_FOLDS)
    assert len(st.DROP_KINDS) == so.ST_DROP_KINDS and len(st.SCORE_FIELDS) == so.ST_SCORE_FIELDS
    assert [so.n_fields(k) for k in (1, 2, 3, 4)] == [6, 10, 15, 21] == [ref.n_fields(k) for k in (1, 2, 3, 4)]
    assert os.path.exists(so.LIB_PATH), "libmmgnn_stack.so is not built (make -C multi-modal-gnn_amd/csrc)"
    nm = next((c for c in ("nm", "llvm-nm", "/opt/rocm/llvm/bin/llvm-nm") if shutil.which(c)), None)
    assert nm is not None, "no nm found (nm, llvm-nm, /opt/rocm/llvm/bin/llvm-nm)"
    out = subprocess.run([nm, "-D", "--defined-only", so.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {s for s in exported if s.startswith("mmg_")} == set(so.SIGNATURES)
