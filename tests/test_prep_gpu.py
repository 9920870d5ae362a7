"""Lab preprocessing on the device (csrc/prep.hip through mmgnn.preprocess) against the reference's results
(tests/golden/prep_small.npz) and, on make_lab_events at x1 and x10, against the restatement prep_ref.py.

Exact (bit-equal): which events leave as outliers, the set and order of the pairs, VALUE for last / min / max / median,
min / max / median / q25 / q75 in the stats, minmax- and robust-normalised values, dtypes.
Sums (mean, std, "mean" aggregation, z-scores): pandas and the kernels add the same fp64 terms in different orders.
The tolerance is not picked by hand: the golden file records how far the REFERENCE's own results lie from a
high-precision evaluation of the same formulas (meta["sum_rel_dev_max"], 2.6e-16 in the committed file, in the
condition-scaled measure of prep_ref.sum_deviations), and the device results may lie 8x that far from the same
evaluation (8x: the kernels' chunk / tree / chunk-row order has a different depth from pandas' loops)."""
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import graph_build, inference, preprocess
from mmgnn.synth import lab_event_frames, make_lab_events
import prep_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prep_small.npz")
CASES = [(k, a, r) for k in ("int", "str") for a in prep_ref.AGGS for r in (True, False)]
EXACT_AGGS = ("last", "median", "min", "max")
FACTOR = 8.0


@pytest.fixture(scope="module")
def gold():
    d = np.load(GOLDEN)
    meta = json.loads(str(d["__meta__"]))
    return d, meta, FACTOR * meta["sum_rel_dev_max"]


def _same_keys(got, want):
    assert np.array_equal(got["SUBJECT_ID"].to_numpy(), want["SUBJECT_ID"].to_numpy())
    assert got["ITEMID"].tolist() == want["ITEMID"].tolist()
    assert got["SUBJECT_ID"].dtype == np.int64


def _zscore_deviation(frame_agg, stats, frame_norm):
    """Condition-scaled deviation of zscore stats and values from the high-precision evaluation (prep_ref)."""
    lc, keys = pd.factorize(frame_agg["ITEMID"], sort=True)
    have = {k: stats[str(key)] for k, key in enumerate(keys) if stats.get(str(key)) is not None}
    gm = {k: s["mean"] for k, s in have.items()}
    gs = {k: s["std"] for k, s in have.items()}
    dev = prep_ref.sum_deviations(lc[np.isin(lc, list(have))], frame_agg["VALUE"].to_numpy()[np.isin(lc, list(have))], gm, gs)
    # the normalised rows: (lab, input order) of the non-NaN values
    order = np.argsort(lc, kind="stable")
    v = frame_agg["VALUE"].to_numpy()[order]
    keep = ~np.isnan(v)
    assert prep_ref.same_bits(v[keep], frame_norm["VALUE"].to_numpy())
    dz = prep_ref.sum_deviations(lc[order][keep], v[keep], got_z=frame_norm["VALUE_NORMALIZED"].to_numpy())
    return dev, dz


@pytest.mark.parametrize("kind,agg,remove", CASES)
def test_frames_match_the_reference(gold, kind, agg, remove):
    d, meta, tol = gold
    labs, cohort = prep_ref.golden_events(d, kind)
    tag = f"{kind}_{agg}_{'on' if remove else 'off'}"
    want = prep_ref.golden_frame(d, f"{tag}_agg", kind)
    got = preprocess.aggregate_lab_values(labs, cohort, agg, remove, meta["threshold"])
    assert list(got.columns) == ["SUBJECT_ID", "ITEMID", "VALUE"]
    _same_keys(got, want)                                       # every pair, in the reference's order
    if agg in EXACT_AGGS:
        assert prep_ref.same_bits(got["VALUE"], want["VALUE"])
    else:
        assert np.array_equal(np.isnan(got["VALUE"]), np.isnan(want["VALUE"]))
        ev = prep_ref.clean_events(labs, cohort["SUBJECT_ID"], remove, meta["threshold"])
        dev = prep_ref.mean_agg_deviation(ev, got)
        print(f"{tag}: mean aggregation deviation {dev:.3e} (allowed {tol:.3e})")
        assert dev <= tol
    for norm in prep_ref.NORMS:
        wn = prep_ref.golden_frame(d, f"{tag}_{norm}", kind)
        gn, nz = preprocess.normalize_lab_values(want, norm)
        assert list(gn.columns) == ["SUBJECT_ID", "ITEMID", "VALUE", "VALUE_NORMALIZED"]
        _same_keys(gn, wn)
        assert gn["ITEMID"].dtype == (np.int64 if kind == "int" else object)
        assert prep_ref.same_bits(gn["VALUE"], wn["VALUE"])
        wstats = meta["stats"][f"{tag}_{norm}"]
        assert set(nz.stats) == set(wstats) and nz.method == norm
        for lab, ws in wstats.items():
            assert (nz.stats[lab] is None) == (ws is None), lab
            if ws is not None:
                assert set(nz.stats[lab]) == set(ws)
                if norm != "zscore":
                    for f, w in ws.items():
                        assert prep_ref.same_bits(nz.stats[lab][f], w), (lab, f)
                else:
                    assert np.isnan(nz.stats[lab]["std"]) == np.isnan(ws["std"])
        if norm == "zscore":
            dev, dz = _zscore_deviation(want, nz.stats, gn)
            print(f"{tag}: zscore stats deviation {dev:.3e}, values {dz:.3e} (allowed {tol:.3e})")
            assert dev <= tol and dz <= tol
        else:
            assert prep_ref.same_bits(gn["VALUE_NORMALIZED"], wn["VALUE_NORMALIZED"])


def test_remove_outliers_matches_the_reference(gold):
    d, meta, _ = gold
    for name, spec in meta["outliers"].items():
        x = d[f"out_{name}_in"]
        got = preprocess.remove_outliers(x, spec["method"], spec["threshold"])
        assert isinstance(got, np.ndarray) and prep_ref.same_bits(got, d[f"out_{name}_out"]), name
        s = preprocess.remove_outliers(pd.Series(x, index=np.arange(len(x)) + 5), spec["method"], spec["threshold"])
        assert isinstance(s, pd.Series) and s.index[0] == 5 and prep_ref.same_bits(s.to_numpy(), got)
        t = preprocess.remove_outliers(torch.from_numpy(x).to(DEV), spec["method"], spec["threshold"])
        assert t.is_cuda and prep_ref.same_bits(t.cpu().numpy(), got)


_EVENTS = {}


def _events(scale):
    if scale not in _EVENTS:
        _EVENTS.clear()
        ev = make_lab_events(scale, seed=0, device=DEV)
        labs, cohort = lab_event_frames(ev)
        inc = labs[labs["SUBJECT_ID"] < ev["n_patients"]]
        margin = min(prep_ref.bound_margin(g, "std", 5.0) for _, g in inc.groupby("ITEMID")["VALUENUM"])
        assert margin > 1e-9, "an event within 1e-9 of an outlier bound: the removal would hang on the last bit"
        _EVENTS[scale] = (ev, labs, cohort)
    return _EVENTS[scale]


@pytest.mark.parametrize("scale,agg,thr,norm", [
    (1, "last", 5.0, "zscore"), (1, "mean", 5.0, "robust"), (1, "median", None, "minmax"), (1, "min", 5.0, "minmax"),
    (1, "max", None, "zscore"), (1, "last", None, "robust"),
    (10, "last", 5.0, "zscore"), (10, "median", 5.0, "robust"), (10, "mean", None, "minmax")])
def test_tensor_level_against_the_restatement(gold, scale, agg, thr, norm):
    _, _, tol = gold
    ev, labs, cohort = _events(scale)
    p, l, v, vn, nz = preprocess.preprocess_lab_events(ev["patient"], ev["lab"], ev["value"], ev["time"], ev["n_patients"],
                                                       ev["n_labs"], aggregate=agg, outlier_threshold=thr, normalize=norm)
    assert p.dtype == l.dtype == torch.int64 and v.dtype == vn.dtype == torch.float64 and p.is_cuda
    ragg = prep_ref.aggregate(labs, cohort, agg, thr is not None, thr if thr is not None else 5.0)
    rn, rstats = prep_ref.normalize(ragg, norm)
    p, l, v, vn = (t.cpu().numpy() for t in (p, l, v, vn))
    assert np.array_equal(p, rn["SUBJECT_ID"].to_numpy()) and np.array_equal(l, rn["ITEMID"].to_numpy())
    if agg in EXACT_AGGS:
        assert prep_ref.same_bits(v, rn["VALUE"])
    else:
        clean = prep_ref.clean_events(labs, cohort["SUBJECT_ID"], thr is not None, thr if thr is not None else 5.0)
        got = pd.DataFrame({"SUBJECT_ID": p, "ITEMID": l, "VALUE": v})
        dev = prep_ref.mean_agg_deviation(clean, got)
        print(f"x{scale} {agg}: mean aggregation deviation {dev:.3e} (allowed {tol:.3e})")
        assert dev <= tol
    assert set(nz.stats) == set(rstats)
    if norm == "zscore":
        gm = {int(k): s["mean"] for k, s in nz.stats.items()}
        gs = {int(k): s["std"] for k, s in nz.stats.items()}
        dev = prep_ref.sum_deviations(l, v, gm, gs, vn)
        print(f"x{scale} {agg}: zscore deviation {dev:.3e} (allowed {tol:.3e})")
        assert dev <= tol
    elif agg in EXACT_AGGS:                                     # bit-equal inputs: bit-equal order statistics and values
        for k, s in rstats.items():
            for f, w in s.items():
                assert prep_ref.same_bits(nz.stats[k][f], w), (k, f)
        assert prep_ref.same_bits(vn, rn["VALUE_NORMALIZED"])
    else:                                                       # "mean" values differ in the last bits: so may quantiles
        for k, s in rstats.items():
            for f, w in s.items():
                assert abs(nz.stats[k][f] - w) <= tol * max(abs(w), 1.0), (k, f)


def test_inverse_round_trip_and_matrix(gold):
    _, _, tol = gold
    ev, _, _ = _events(1)
    L = ev["n_labs"]
    for norm in prep_ref.NORMS:
        p, l, v, vn, nz = preprocess.preprocess_lab_events(ev["patient"], ev["lab"], ev["value"], ev["time"],
                                                           ev["n_patients"], L, normalize=norm)
        worst = 0.0
        for k in (0, 7, L - 1):
            sel = l == k
            back = nz.inverse_transform(vn[sel], str(k))
            assert back.dtype == torch.float64
            worst = max(worst, float(((back - v[sel]).abs() / v[sel].abs().max()).max()))
            # pandas in, pandas out
            s = nz.inverse_transform(pd.Series(vn[sel].cpu().numpy()), str(k))
            assert isinstance(s, pd.Series) and prep_ref.same_bits(s.to_numpy(), back.cpu().numpy())
            assert prep_ref.same_bits(nz.transform(v[sel], str(k)).cpu().numpy(), vn[sel].cpu().numpy())
        print(f"{norm}: inverse(transform(v)) deviates by {worst:.3e} of max|v| (allowed {tol:.3e})")
        assert worst <= tol
        wide = torch.randn(257, L + 6, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
        pred = wide[:, 3:3 + L]                                 # a leading dimension, as impute_lab_matrix's result has
        full = nz.inverse_transform_matrix(pred)
        assert full.shape == pred.shape and full.dtype == torch.float32
        for k in range(L):
            col = nz.inverse_transform(pred[:, k].contiguous(), str(k))
            assert col.dtype == torch.float32 and torch.equal(col, full[:, k]), (norm, k)
        want = prep_ref.inverse(pred[:, 5].double().cpu().numpy(), nz.stats["5"], norm).astype(np.float32)
        assert np.array_equal(full[:, 5].cpu().numpy(), want)


def test_two_runs_are_bitwise_equal_at_x10():
    ev, _, _ = _events(10)
    runs = []
    for _ in range(2):
        p, l, v, vn, nz = preprocess.preprocess_lab_events(ev["patient"], ev["lab"], ev["value"], ev["time"],
                                                           ev["n_patients"], ev["n_labs"], "mean", 5.0, "robust")
        runs.append((p, l, v.view(torch.int64), vn.view(torch.int64), json.dumps(nz.stats, sort_keys=True)))
    for a, b in zip(*runs):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    assert runs[0][0].numel() > 600_000


def test_empty_and_nothing_survives():
    z = torch.zeros(0, dtype=torch.int64, device=DEV)
    p, l, v, vn, nz = preprocess.preprocess_lab_events(z, z, z.double(), z, 5, 3)
    assert p.numel() == l.numel() == v.numel() == vn.numel() == 0 and nz.stats == {}
    pat = torch.tensor([7, -1, 9, 2], device=DEV)               # nobody in the cohort, or no selected lab
    lab = torch.tensor([0, 1, 2, 5], device=DEV)
    val = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64, device=DEV)
    for agg in prep_ref.AGGS:
        p, l, v, vn, nz = preprocess.preprocess_lab_events(pat, lab, val, lab, 5, 3, aggregate=agg)
        assert p.numel() == 0 and nz.stats == {}
    nanv = torch.full((4,), float("nan"), dtype=torch.float64, device=DEV)
    p, l, v, vn, nz = preprocess.preprocess_lab_events(lab % 3, lab % 3, nanv, lab, 5, 3, outlier_threshold=None)
    assert p.numel() == 0 and set(nz.stats) == {"0", "1", "2"} and nz.stats["0"] is None


def test_end_to_end_frames_to_graph_edges(gold):
    _, _, tol = gold
    ev, labs, cohort = _events(1)
    agg = preprocess.aggregate_lab_values(labs, cohort, "last", True, 5.0)
    norm, nz = preprocess.normalize_lab_values(agg, "zscore")
    ragg = prep_ref.aggregate(labs, cohort, "last", True, 5.0)
    rnorm, _ = prep_ref.normalize(ragg, "zscore")
    _same_keys(agg, ragg)
    assert prep_ref.same_bits(agg["VALUE"], ragg["VALUE"])
    edges = []
    for frame in (norm, rnorm):
        pix, lix = graph_build.NodeIndexer(), graph_build.NodeIndexer()
        pix.add_many(cohort["SUBJECT_ID"])
        lix.add_many(frame["ITEMID"])
        edges.append(graph_build.create_patient_lab_edges(frame, pix, lix) + (lix,))
    (ei, ea, lix), (rei, rea, _) = edges
    assert torch.equal(ei, rei) and ei.shape[1] == len(rnorm) == ev["edge_index"].shape[1]
    # float32 edge values: equal except where the two fp64 z-scores straddle a float32 rounding boundary.  Each may lie
    # d_i = tol * (max|v| / std + |z|) from the exact z, so they differ by at most 2 d_i, and a boundary (one per float32
    # ulp) falls between them with probability <= 2 d_i / ulp32(z_i); the count is held to that expectation plus four
    # standard deviations of a Poisson count, plus one.
    z = rnorm["VALUE_NORMALIZED"].to_numpy()
    cond = np.empty(len(z))
    lc = rnorm["ITEMID"].to_numpy()
    for k in np.unique(lc):
        sel = lc == k
        v = rnorm["VALUE"].to_numpy()[sel]
        cond[sel] = np.abs(v).max() / v.std(ddof=1) + np.abs(z[sel])
    ulp32 = np.spacing(np.abs(z).astype(np.float32)).astype(np.float64)
    lam = float(np.sum(np.minimum(1.0, 2 * tol * cond / ulp32)))
    allowed = int(np.ceil(lam + 4 * np.sqrt(lam) + 1))
    differ = int((ea != rea).sum())
    print(f"end to end: {differ} of {len(z)} float32 edge values differ (expected {lam:.3f}, allowed {allowed})")
    assert differ <= allowed
    assert float((ea - rea).abs().max()) <= float(ulp32.max())
    # the normaliser drives inference.lab_report unchanged
    stats = nz.to_lab_stats()
    sid = int(norm["SUBJECT_ID"].iloc[0])
    mine = norm[norm["SUBJECT_ID"] == sid]
    lab_idx = np.array([lix.get_index(i) for i in mine["ITEMID"]])
    pred_row = np.linspace(-1, 1, len(lix)).astype(np.float32)
    rep = inference.lab_report(pred_row, lab_idx, mine["VALUE_NORMALIZED"].to_numpy(np.float32),
                               np.arange(len(mine)) % 2 == 0, stats, lix.id_to_index)
    assert len(rep["measured_labs"]) + len(rep["masked_labs"]) == len(mine)
    assert len(rep["truly_missing_labs"]) == len(lix) - len(mine)
    name = lix.get_id(int(lab_idx[1]))
    want = float(mine["VALUE"].iloc[1])
    assert abs(rep["measured_labs"][name]["value"] - want) <= 1e-6 * abs(want)
