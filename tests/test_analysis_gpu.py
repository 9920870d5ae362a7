"""Prediction analysis on the MI355X (mmg_pair_analysis / mmg_pair_calibrated_abs, mmgnn/analysis.py): the device
tables against the float64 evaluation of analysis_ref.py under its recorded bounds (no further from it than the
reference's own recipe is), exact counts / rows / flags, bitwise reproducibility (int64 against int32 indices, run
against run, eager against a replayed hipGraph), shuffled pairs, run_analysis end to end, and what the whole
population shows that a 10,000-pair sample does not."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import analysis, ops
from mmgnn._lib import MmgError
from mmgnn.model import build_model
from mmgnn.synth import make_graph
from mmgnn.train import LAB_EDGE
import analysis_ref as ar

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_CACHE = {}


def _case(scale):
    """(graph on the device, device tensors pred / target / patient / lab, their numpy copies, host degrees)"""
    if scale not in _CACHE:
        g = make_graph(scale, seed=0)
        p, t, pi, li, _, _ = ar.inputs(g)
        dev = tuple(torch.from_numpy(x).to(DEV) for x in (p, t, pi, li))
        _CACHE[scale] = (g.to(DEV), dev, (p, t, pi, li), ar.degrees(g))
    return _CACHE[scale]


def _check(name, table, got, want, cols, bounds, key=None):
    for c in cols:
        d = ar.distance(got, want, c, key)
        print(f"{name} {table}.{c}: distance {d:.3e} (allowed {bounds[table + '.' + c]:.3e})")
        assert d <= bounds[table + "." + c], (name, table, c, d)


@pytest.mark.parametrize("scale", [1, 100])
def test_device_tables_against_float64_evaluation(scale):
    g, (p, t, pi, li), (hp, ht, hpi, hli), deg = _case(scale)
    bounds = ar.BOUNDS[f"x{scale}"]
    tb = analysis.analysis_tables(p, t, pi, li, g)
    cal, want = tb["calibration"], ar.calibration_f64(hp, ht, hli)
    # exact: which labs, their order, counts, the flag (the thresholds are further away than the bound: checked on the
    # float64 evaluation, so the comparison cannot pass or fail by luck)
    assert min(np.abs(np.abs(want["a"] - 1) - 0.1).min(), np.abs(np.abs(want["b"]) - 0.1).min()) > 10 * bounds["calibration.a"]
    assert list(cal["lab_idx"]) == list(want["lab_idx"])
    assert list(cal["n_samples"]) == list(want["n_samples"])
    assert list(cal["is_calibrated"]) == list(want["is_calibrated"])
    assert list(cal["lab_name"]) == list(want["lab_name"])
    _check(f"x{scale}", "calibration", cal, want, ar.CAL_FLOAT, bounds, "lab_idx")
    dg, want = tb["error_vs_degree"], ar.degree_f64(hp, ht, hpi, deg)
    assert list(dg["degree_bin"]) == list(want["degree_bin"]) and list(dg["count"]) == list(want["count"])
    _check(f"x{scale}", "degree", dg, want, ar.DEG_FLOAT, bounds)
    dc, want = tb["parity_by_decile"], ar.deciles_f64(hp, ht, hli)
    for c in ("decile", "n_labs", "count_min", "count_max", "n_pairs"):
        assert list(dc[c]) == list(want[c]), c
    _check(f"x{scale}", "decile", dc, want, ar.DEC_FLOAT, bounds)
    # the single-table entry points read the same sums
    one = analysis.create_per_lab_calibration_table(p, t, li, None)
    for c in ar.CAL_FLOAT:
        assert ar.distance(one, cal, c, "lab_idx") <= bounds["calibration." + c]
    pd.testing.assert_frame_equal(analysis.parity_by_frequency_decile(p, t, li), dc)


def test_open_ended_bins_keep_high_degree_patients():
    g, (p, t, pi, li), (hp, ht, hpi, hli), deg = _case(1)
    closed = analysis.create_error_vs_degree_table(p, t, pi, g)
    opened = analysis.create_error_vs_degree_table(p, t, pi, g, bins=(0, 1, 6, 16, np.inf))
    assert int(closed["count"].sum()) == 61484 - 9700 and int(opened["count"].sum()) == 61484
    want = ar.degree_f64(hp, ht, hpi, deg, bins=(0, 1, 6, 16, np.inf))
    assert list(opened["count"]) == list(want["count"])
    _check("x1 open", "degree", opened, want, ar.DEG_FLOAT, ar.BOUNDS["x1"])


def _sums(p, t, pi, li, deg, edges=(0.0, 1.0, 6.0, 16.0, 50.0), n_labs=50):
    ls, bs = ops.pair_analysis(p, t, li, n_labs, pi, deg, edges)
    a = torch.linspace(0.8, 1.2, n_labs, device=DEV)
    b = torch.linspace(-0.2, 0.2, n_labs, device=DEV)
    mean = (bs[:, 1] / bs[:, 0].clamp(min=1)).contiguous()
    la, bq = ops.pair_calibrated_abs(p, t, li, a, b, pi, deg, edges, mean)
    return [x.clone() for x in (ls, bs, la, bq)]


def _bits(xs):
    return [x.cpu().numpy().view(np.int64).copy() for x in xs]


@pytest.mark.parametrize("scale", [1, 100])
def test_bitwise_reproducible_int32_and_captured(scale):
    g, (p, t, pi, li), _, deg = _case(scale)
    d = torch.from_numpy(deg.astype(np.int32)).to(DEV)
    ref = _bits(_sums(p, t, pi, li, d))
    again = _bits(_sums(p, t, pi, li, d))
    narrow = _bits(_sums(p, t, pi.to(torch.int32), li.to(torch.int32), d))
    for r, a, b in zip(ref, again, narrow):
        assert np.array_equal(r, a), "two runs differ"
        assert np.array_equal(r, b), "int32 and int64 indices differ"
    # captured and replayed twice: no memset node, no allocation, no host synchronisation inside the two entry points
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _sums(p, t, pi, li, d)                           # warm-up off the default stream, as torch.cuda.graph asks
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _sums(p, t, pi, li, d)
    for _ in range(2):
        for o in outs:
            o.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        for r, o in zip(ref, _bits(outs)):
            assert np.array_equal(r, o), "a replayed capture differs from the eager run"


def test_shuffled_pairs_within_the_bound():
    """A different order of the pairs is a different (fixed) order of the fp64 additions: the tables agree within the
    bound, not bit for bit."""
    g, (p, t, pi, li), (hp, ht, hpi, hli), deg = _case(1)
    perm = torch.randperm(p.numel(), generator=torch.Generator().manual_seed(3)).to(DEV)
    tb = analysis.analysis_tables(p[perm].contiguous(), t[perm].contiguous(), pi[perm].contiguous(),
                                  li[perm].contiguous(), g)
    b = ar.BOUNDS["x1"]
    _check("shuffled", "calibration", tb["calibration"], ar.calibration_f64(hp, ht, hli), ar.CAL_FLOAT, b, "lab_idx")
    _check("shuffled", "degree", tb["error_vs_degree"], ar.degree_f64(hp, ht, hpi, deg), ar.DEG_FLOAT, b)
    _check("shuffled", "decile", tb["parity_by_decile"], ar.deciles_f64(hp, ht, hli), ar.DEC_FLOAT, b)


def test_edge_cases_on_the_device():
    # lab 0: one pair (left out); lab 1: constant targets; lab 2: ordinary; lab 3: absent; bins with 0 and 1 pair
    p = np.array([1.0, 2.0, 2.5, 3.5, 0.1, 0.9, 2.2, 2.9], np.float32)
    t = np.array([1.5, 0.1, 0.1, 0.1, 0.0, 1.0, 2.0, 3.0], np.float32)
    li = np.array([0, 1, 1, 1, 2, 2, 2, 2])
    pi = np.array([0, 1, 1, 1, 2, 2, 2, 2])
    deg = np.array([1, 7, 60], np.int32)                   # patient 2: degree >= 50, dropped under the default bins
    dev = [torch.from_numpy(x).to(DEV) for x in (p, t, pi, li)]
    cal = analysis.create_per_lab_calibration_table(dev[0], dev[1], dev[3], {1: "flat"})
    want = ar.calibration_f64(p, t, li, {1: "flat"})
    assert list(cal["lab_idx"]) == list(want["lab_idx"]) == [1, 2]
    row = cal[cal["lab_idx"] == 1].iloc[0]
    assert row["a"] == 0.0 and row["b"] == pytest.approx(8.0 / 3.0, abs=1e-12) and row["lab_name"] == "flat"
    for c in ar.CAL_FLOAT:
        assert ar.distance(cal, want, c, "lab_idx") <= 1e-12
    dg = analysis.create_error_vs_degree_table(dev[0], dev[1], dev[2], torch.from_numpy(deg).to(DEV))
    assert list(dg["count"]) == [0, 1, 3, 0]
    assert np.isnan(dg["mean"][0]) and np.isnan(dg["std"][0]) and np.isnan(dg["std"][1]) and dg["mean"][1] == 0.5
    want = ar.degree_f64(p, t, pi, deg)
    for c in ar.DEG_FLOAT:
        assert ar.distance(dg, want, c) <= 1e-12
    dc = analysis.parity_by_frequency_decile(dev[0], dev[1], dev[3])
    want = ar.deciles_f64(p, t, li)
    assert list(dc["decile"]) == list(want["decile"]) and list(dc["n_pairs"]) == list(want["n_pairs"])
    for c in ar.DEC_FLOAT:
        assert ar.distance(dc, want, c) <= 1e-12
    # indices outside the tables are counted nowhere and never used as an address
    bad = torch.tensor([-1, 5, 1 << 40, 2], device=DEV)
    ls, bs = ops.pair_analysis(dev[0][:4].contiguous(), dev[1][:4].contiguous(), bad, 3, bad,
                               torch.from_numpy(deg).to(DEV), (0.0, 100.0))
    assert ls[:, 0].tolist() == [0.0, 0.0, 1.0] and bs[:, 0].tolist() == [1.0]


def test_many_labs_on_the_device_and_beyond():
    rng = np.random.default_rng(5)
    n, labs = 200_000, 2048
    li = rng.integers(0, labs, n)
    t = rng.standard_normal(n).astype(np.float32)
    p = (t * 0.9 + 0.05 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    dp, dt, dl = (torch.from_numpy(x).to(DEV) for x in (p, t, li))
    ls, _ = ops.pair_analysis(dp, dt, dl, labs)
    host, _ = analysis._first_read_host(p, t, li, labs, None, None, None)
    assert np.array_equal(ls[:, 0].cpu().numpy(), host[:, 0])
    assert np.allclose(ls.cpu().numpy(), host, rtol=1e-12, atol=1e-12)
    # one lab more than the device tables hold: the entry point refuses, the module falls back to the host arithmetic
    li2 = li.copy()
    li2[0] = labs
    with pytest.raises(MmgError, match="2049 labs"):
        ops.pair_analysis(dp, dt, torch.from_numpy(li2).to(DEV), labs + 1)
    cal = analysis.create_per_lab_calibration_table(dp, dt, torch.from_numpy(li2).to(DEV), None)
    want = ar.calibration_f64(p, t, li2)
    assert list(cal["lab_idx"]) == list(want["lab_idx"])
    for c in ar.CAL_FLOAT:
        assert ar.distance(cal, want, c, "lab_idx") <= 1e-9


def test_run_analysis_end_to_end(tmp_path):
    g = make_graph(1, seed=0).to(DEV)
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"}}
    torch.manual_seed(0)
    model = build_model(cfg, (g.node_types, g.edge_types), None).to(DEV)
    model._init_embeddings(g)
    cal, dg, dc = analysis.run_analysis(model, g, output_dir=tmp_path)
    for f in ("per_lab_calibration.csv", "error_vs_degree.csv", "parity_by_frequency_decile.csv"):
        assert os.path.getsize(tmp_path / f) > 0
    ei, y = g[LAB_EDGE].edge_index, g[LAB_EDGE].edge_attr.reshape(-1)
    model.eval()
    with torch.no_grad():
        pred = model.predict_lab_values(g, ei[0].contiguous(), ei[1].contiguous()).reshape(-1)
    tb = analysis.analysis_tables(pred, y, ei[0], ei[1], g, n_labs=50)
    pd.testing.assert_frame_equal(cal, tb["calibration"])
    pd.testing.assert_frame_equal(dg, tb["error_vs_degree"])
    pd.testing.assert_frame_equal(dc, tb["parity_by_decile"])
    assert int(cal["n_samples"].sum()) == 61484 and int(dc["n_pairs"].sum()) == 61484
    back = pd.read_csv(tmp_path / "per_lab_calibration.csv")
    assert list(back.columns) == analysis.CALIBRATION_COLUMNS and len(back) == len(cal)


def test_whole_population_against_a_10000_pair_sample():
    """What the feature is for, on counts only: the reference keeps 10,000 of the x100 graph's 6.1 M pairs, so its table
    of the rarest labs rests on ~1/600 of their pairs."""
    g, (p, t, pi, li), _, _ = _case(100)
    full = analysis.create_per_lab_calibration_table(p, t, li, None)
    idx = torch.from_numpy(np.random.default_rng(0).choice(p.numel(), 10000, replace=False)).to(DEV)
    part = analysis.create_per_lab_calibration_table(p[idx].contiguous(), t[idx].contiguous(), li[idx].contiguous(), None)
    rare = full.sort_values("n_samples")["lab_idx"][:5]
    nf = full.set_index("lab_idx")["n_samples"]
    ns = part.set_index("lab_idx")["n_samples"].reindex(rare).fillna(0)
    assert int(full["n_samples"].sum()) == p.numel() and int(part["n_samples"].sum()) <= 10000
    for lab in rare:
        assert nf[lab] > 50_000 and ns[lab] < 300, (lab, nf[lab], ns[lab])
