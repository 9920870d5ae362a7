"""Prediction analysis without a GPU: the float64 evaluation of analysis_ref.py against the reference's own
mixed-precision recipe (where the allowed distances are measured, and compared with what analysis_ref.BOUNDS records),
the host path of mmgnn.analysis against that evaluation, the CSV, the edge cases, and the argument errors of the two
new entry points."""
import ctypes
import logging

import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import analysis
from mmgnn.synth import make_graph
import analysis_ref as ar


@pytest.fixture(scope="module")
def x1():
    g = make_graph(1, seed=0)
    p, t, pi, li, slope, offset = ar.inputs(g)
    return g, p, t, pi, li, ar.degrees(g), slope, offset


def _tables_close(tb, p, t, pi, li, deg, bounds, bins=ar.BINS):
    cal, want = tb["calibration"], ar.calibration_f64(p, t, li)
    assert list(cal["lab_idx"]) == list(want["lab_idx"]) and list(cal["n_samples"]) == list(want["n_samples"])
    assert list(cal["is_calibrated"]) == list(want["is_calibrated"])
    for c in ar.CAL_FLOAT:
        assert ar.distance(cal, want, c, "lab_idx") <= bounds["calibration." + c], c
    dg, want = tb["error_vs_degree"], ar.degree_f64(p, t, pi, deg, bins)
    assert list(dg["count"]) == list(want["count"])
    for c in ar.DEG_FLOAT:
        assert ar.distance(dg, want, c) <= bounds["degree." + c], c
    dc, want = tb["parity_by_decile"], ar.deciles_f64(p, t, li)
    for c in ("decile", "n_labs", "count_min", "count_max", "n_pairs"):
        assert list(dc[c]) == list(want[c]), c
    for c in ar.DEC_FLOAT:
        assert ar.distance(dc, want, c) <= bounds["decile." + c], c


def _assert_recorded(name, p, t, pi, li, deg):
    measured = ar.measure_bounds(p, t, pi, li, deg)
    assert set(measured) == set(ar.BOUNDS[name])
    for c, d in measured.items():
        rec = ar.BOUNDS[name][c]
        print(f"{name} {c}: measured {d:.4e}, recorded {rec:.3e}")
        assert 0 < d <= rec <= 1.01 * d, (name, c, d, rec)


def test_recorded_bounds_are_the_measured_distances(x1):
    """The distance of the reference's recipe (sklearn LinearRegression on fp32, fp32 np.mean, pandas on an fp32 column)
    from the float64 evaluation, per column, is what analysis_ref.BOUNDS["x1"] records (rounded up to three digits)."""
    pytest.importorskip("sklearn")
    g, p, t, pi, li, deg, _, _ = x1
    _assert_recorded("x1", p, t, pi, li, deg)


def test_recorded_bounds_at_x100_are_the_measured_distances():
    """The same for BOUNDS["x100"], which the GPU test of the 6.1 M-pair graph relies on (about a quarter of a minute)."""
    pytest.importorskip("sklearn")
    g = make_graph(100, seed=0)
    p, t, pi, li, _, _ = ar.inputs(g)
    _assert_recorded("x100", p, t, pi, li, ar.degrees(g))
    f = ar.calibration_f64(p, t, li)
    margin = min(np.abs(np.abs(f["a"] - 1) - 0.1).min(), np.abs(np.abs(f["b"]) - 0.1).min())
    assert margin > 1e-3 > 1000 * max(ar.BOUNDS["x100"].values())


def test_known_answers_and_threshold_margins(x1):
    g, p, t, pi, li, deg, slope, offset = x1
    f = ar.calibration_f64(p, t, li).sort_values("lab_idx")
    assert np.abs(f["a"].values - slope).max() < 0.03 and np.abs(f["b"].values - offset).max() < 0.03
    # every lab is further from both is_calibrated thresholds than any bound: the exact comparison of the flag is safe
    margin = min(np.abs(np.abs(f["a"] - 1) - 0.1).min(), np.abs(np.abs(f["b"]) - 0.1).min())
    assert margin > 1e-3 > 1000 * max(ar.BOUNDS["x1"].values())
    assert 0 < f["is_calibrated"].sum() < len(f)
    assert ar.deciles_f64(p, t, li).shape[0] == 10


def test_host_path_against_float64_evaluation(x1):
    g, p, t, pi, li, deg, _, _ = x1
    tb = analysis.analysis_tables(p, t, pi, li, g)
    _tables_close(tb, p, t, pi, li, deg, ar.BOUNDS["x1"])
    # tensors on the host and the single-table entry points give the same tables
    cal = analysis.create_per_lab_calibration_table(torch.from_numpy(p), torch.from_numpy(t), torch.from_numpy(li), None)
    pd.testing.assert_frame_equal(cal, tb["calibration"])
    pd.testing.assert_frame_equal(analysis.create_error_vs_degree_table(p, t, pi, g), tb["error_vs_degree"])
    pd.testing.assert_frame_equal(analysis.parity_by_frequency_decile(p, t, li), tb["parity_by_decile"])
    assert list(tb["calibration"].columns) == analysis.CALIBRATION_COLUMNS
    assert list(tb["error_vs_degree"].columns) == analysis.DEGREE_COLUMNS
    assert list(tb["parity_by_decile"].columns) == analysis.DECILE_COLUMNS
    assert tb["calibration"]["mae_before"].is_monotonic_decreasing


def test_degree_quirk_and_open_bins(x1, caplog):
    g, p, t, pi, li, deg, _, _ = x1
    assert int((deg >= 50).sum()) == 194
    with caplog.at_level(logging.INFO):
        closed = analysis.create_error_vs_degree_table(p, t, pi, g)
    assert "9700 of 61484 pairs fall into no degree bin" in caplog.text
    assert int(closed["count"].sum()) == 61484 - 9700
    opened = analysis.create_error_vs_degree_table(p, t, pi, g, bins=(0, 1, 6, 16, np.inf))
    assert int(opened["count"].sum()) == 61484
    want = ar.degree_f64(p, t, pi, deg, bins=(0, 1, 6, 16, np.inf))
    assert list(opened["count"]) == list(want["count"])
    for c in ar.DEG_FLOAT:
        assert ar.distance(opened, want, c) <= ar.BOUNDS["x1"]["degree." + c]


def test_csv_columns_order_and_format(x1, tmp_path):
    g, p, t, pi, li, deg, _, _ = x1
    df = analysis.create_per_lab_calibration_table(p, t, li, {0: "sodium"}, output_dir=tmp_path)
    lines = (tmp_path / "per_lab_calibration.csv").read_text().splitlines()
    assert lines[0] == "lab_idx,lab_name,n_samples,a,b,mae_before,mae_after,delta_mae,is_calibrated"
    assert len(lines) == 1 + len(df)
    first = lines[1].split(",")
    r = df.iloc[0]
    assert first[0] == str(r["lab_idx"]) and first[2] == str(r["n_samples"]) and first[8] == str(bool(r["is_calibrated"]))
    assert first[3:8] == ["%.4f" % r[c] for c in ("a", "b", "mae_before", "mae_after", "delta_mae")]
    assert "sodium" in df["lab_name"].values and "Lab_1" in df["lab_name"].values


def test_edge_cases():
    # lab 0: one pair (left out); lab 1: constant targets; lab 2: ordinary; lab 3: absent
    p = np.array([1.0, 2.0, 2.5, 3.5, 0.1, 0.9, 2.2, 2.9], np.float32)
    t = np.array([1.5, 0.1, 0.1, 0.1, 0.0, 1.0, 2.0, 3.0], np.float32)
    li = np.array([0, 1, 1, 1, 2, 2, 2, 2])
    pi = np.array([0, 1, 1, 1, 2, 2, 2, 2])
    deg = np.array([1, 7, 60])
    cal = analysis.create_per_lab_calibration_table(p, t, li, {})
    want = ar.calibration_f64(p, t, li)
    assert list(cal["lab_idx"]) == list(want["lab_idx"]) == [1, 2]
    flat = cal[cal["lab_idx"] == 1].iloc[0]
    assert flat["a"] == 0.0 and flat["b"] == pytest.approx(8.0 / 3.0, abs=1e-12)
    for c in ar.CAL_FLOAT:
        assert ar.distance(cal, want, c, "lab_idx") <= 1e-12
    # a bin with no pair and a bin with one: NaN, NaN, 0 and mean, NaN, 1; degree 60 is dropped
    dg = analysis.create_error_vs_degree_table(p, t, pi, deg)
    want = ar.degree_f64(p, t, pi, deg)
    assert list(dg["count"]) == list(want["count"]) == [0, 1, 3, 0]
    assert np.isnan(dg["mean"][0]) and np.isnan(dg["std"][0]) and dg["mean"][1] == 0.5 and np.isnan(dg["std"][1])
    for c in ar.DEG_FLOAT:
        assert ar.distance(dg, want, c) <= 1e-12
    # three labs, two distinct counts: qcut drops duplicate edges and forms fewer than 10 deciles
    dc = analysis.parity_by_frequency_decile(p, t, li)
    want = ar.deciles_f64(p, t, li)
    assert 0 < len(dc) < 10 and list(dc["decile"]) == list(want["decile"])
    for c in ("n_labs", "count_min", "count_max", "n_pairs"):
        assert list(dc[c]) == list(want[c])
    for c in ar.DEC_FLOAT:
        assert ar.distance(dc, want, c) <= 1e-12
    # a decile of constant targets: the bare 1 - SS_res / SS_tot, -inf as numpy gives it
    tc = np.array([0.1, 0.1, 0.1, 0.7, 0.7, 0.7, 0.7], np.float32)
    lc = np.array([1, 1, 1, 2, 2, 2, 2])
    only = analysis.parity_by_frequency_decile(tc + np.float32(0.5), tc, lc)
    assert len(only) == 2 and list(only["r2"]) == [-np.inf, -np.inf]
    assert list(ar.deciles_f64(tc + np.float32(0.5), tc, lc)["r2"]) == [-np.inf, -np.inf]
    assert analysis.parity_by_frequency_decile(tc, tc, lc)["r2"].isna().all()
    # one distinct lab count: qcut forms no decile at all
    assert len(analysis.parity_by_frequency_decile(p[1:4], t[1:4], li[1:4])) == 0
    assert len(ar.deciles_f64(p[1:4], t[1:4], li[1:4])) == 0


def test_empty_and_mismatched_inputs():
    e32, ei = np.zeros(0, np.float32), np.zeros(0, np.int64)
    cal = analysis.create_per_lab_calibration_table(e32, e32, ei, {})
    assert len(cal) == 0 and list(cal.columns) == analysis.CALIBRATION_COLUMNS
    dg = analysis.create_error_vs_degree_table(e32, e32, ei, np.array([3, 4]))
    assert list(dg["count"]) == [0, 0, 0, 0] and dg["mean"].isna().all() and dg["std"].isna().all()
    dc = analysis.parity_by_frequency_decile(e32, e32, ei)
    assert len(dc) == 0 and list(dc.columns) == analysis.DECILE_COLUMNS
    x = np.zeros(4, np.float32)
    with pytest.raises(ValueError):
        analysis.create_per_lab_calibration_table(x, x[:3], np.zeros(4, np.int64), {})
    with pytest.raises(ValueError):
        analysis.create_error_vs_degree_table(x, x, np.zeros(3, np.int64), np.array([1]))
    with pytest.raises(ValueError):
        analysis.parity_by_frequency_decile(x, x, np.zeros(5, np.int64))
    with pytest.raises(ValueError):
        analysis.create_error_vs_degree_table(x, x, np.zeros(4, np.int64), np.array([1]), bins=(0, 5, 5), labels=("a", "b"))


def test_sharded_model_is_refused():
    class Sharded:
        _comm = object()
    with pytest.raises(NotImplementedError, match="dist.shard_model"):
        analysis.run_analysis(Sharded(), None)


def test_package_exports():
    assert mmgnn.run_analysis is analysis.run_analysis
    assert mmgnn.create_per_lab_calibration_table is analysis.create_per_lab_calibration_table


def test_c_abi_argument_errors_without_a_gpu():
    from mmgnn import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nul = ctypes.c_void_p(None)
    ok = (ctypes.c_double * 5)(0, 1, 6, 16, 50)
    bad = (ctypes.c_double * 5)(0, 1, 1, 16, 50)
    big = 1 << 26
    A, W = lib.mmg_pair_analysis, lib.mmg_pair_analysis_ws_bytes
    assert W(1000, 50, 4) > 0 and W(1000, 2048, 4) > 0 and W(1000, 2049, 4) == 0 and W(1000, 50, 65) == 0
    assert W(1000, 2048, 64) == 0 and W(1000, 0, 0) == 0                       # 2048 labs and 64 bins exceed the LDS
    assert A(p, p, p, p, 8, 10, 2049, p, 4, ok, 4, p, p, p, big, nul) == -1     # more labs than the tables hold
    assert b"2049 labs" in lib.mmg_last_error()
    assert A(p, p, p, p, 8, 10, 50, p, 4, ok, 65, p, p, p, big, nul) == -1      # too many bins
    assert A(p, p, p, p, 8, 10, 50, p, 4, bad, 4, p, p, p, big, nul) == -1      # edges not ascending
    assert b"ascending" in lib.mmg_last_error()
    assert A(p, p, p, p, 2, 10, 50, p, 4, ok, 4, p, p, p, big, nul) == -1       # int16 indices
    assert A(p, p, p, p, 8, -1, 50, p, 4, ok, 4, p, p, p, big, nul) == -1       # n < 0
    assert A(p, p, p, nul, 8, 10, 50, p, 4, ok, 4, p, p, p, big, nul) == -1     # null lab indices
    assert A(p, p, nul, p, 8, 10, 50, p, 4, ok, 4, p, p, p, big, nul) == -1     # bins without patient indices
    assert A(p, p, p, p, 8, 10, 0, p, 4, ok, 0, p, p, p, big, nul) == -1        # nothing requested
    assert A(p, p, p, p, 8, 10, 2048, p, 4, ok, 64, p, p, p, big, nul) == -1    # LDS
    assert A(p, p, p, p, 8, 10, 50, p, 4, ok, 4, p, p, p, 16, nul) == -3        # workspace
    assert b"workspace" in lib.mmg_last_error()
    B, WB = lib.mmg_pair_calibrated_abs, lib.mmg_pair_calibrated_abs_ws_bytes
    assert WB(1000, 50, 4) > 0 and WB(1000, 2049, 0) == 0
    assert B(p, p, p, p, 8, 10, 2049, p, p, p, 4, ok, 4, p, p, p, p, big, nul) == -1
    assert B(p, p, p, p, 8, 10, 50, nul, p, p, 4, ok, 4, p, p, p, p, big, nul) == -1   # labs without a
    assert B(p, p, p, p, 8, 10, 50, p, p, p, 4, ok, 4, nul, p, p, p, big, nul) == -1   # bins without their means
    assert B(p, p, p, p, 8, 10, 50, p, p, p, 4, bad, 4, p, p, p, p, big, nul) == -1
    assert B(p, p, p, p, 8, 10, 50, p, p, p, 4, ok, 4, p, p, p, p, 16, nul) == -3
