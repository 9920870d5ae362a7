"""Lab preprocessing on the host: the numpy / pandas restatement (prep_ref.py) against what the reference's own
aggregate_lab_values / normalize_lab_values / remove_outliers returned (tests/golden/prep_small.npz), the C-ABI argument
checks of every entry point of csrc/prep.hip, the ValueErrors, the event generator, and the edges built from the
restatement's frames."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import graph_build, preprocess
from mmgnn.synth import lab_event_frames, make_lab_events
import prep_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prep_small.npz")
CASES = [(k, a, r) for k in ("int", "str") for a in prep_ref.AGGS for r in (True, False)]
EXACT_AGGS = ("last", "median", "min", "max")
# the restatement calls the same pandas reductions as the reference; across numpy builds the order of a pairwise sum
# may differ, so sum-type results are held to a few ulps rather than to the bit
SUM_REL = 1e-13


@pytest.fixture(scope="module")
def gold():
    d = np.load(GOLDEN)
    return d, json.loads(str(d["__meta__"]))


def _same_keys(got, want):
    assert np.array_equal(got["SUBJECT_ID"].to_numpy(), want["SUBJECT_ID"].to_numpy())
    assert got["ITEMID"].tolist() == want["ITEMID"].tolist()
    assert got["SUBJECT_ID"].dtype == np.int64


def _close(a, b, rel):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    assert np.all(np.abs(a[ok] - b[ok]) <= rel * np.maximum(np.abs(b[ok]), 1e-300) + 0.0) or np.allclose(a[ok], b[ok], rtol=rel, atol=1e-14)


@pytest.mark.parametrize("kind,agg,remove", CASES)
def test_restatement_matches_the_reference(gold, kind, agg, remove):
    d, meta = gold
    labs, cohort = prep_ref.golden_events(d, kind)
    tag = f"{kind}_{agg}_{'on' if remove else 'off'}"
    want = prep_ref.golden_frame(d, f"{tag}_agg", kind)
    got = prep_ref.aggregate(labs, cohort, agg, remove, meta["threshold"])
    _same_keys(got, want)
    if agg in EXACT_AGGS:
        assert prep_ref.same_bits(got["VALUE"], want["VALUE"])
    else:
        _close(got["VALUE"], want["VALUE"], SUM_REL)
    for norm in prep_ref.NORMS:
        wn = prep_ref.golden_frame(d, f"{tag}_{norm}", kind)
        gn, stats = prep_ref.normalize(want, norm)
        _same_keys(gn, wn)
        assert gn["ITEMID"].dtype == (np.int64 if kind == "int" else object)
        assert prep_ref.same_bits(gn["VALUE"], wn["VALUE"])
        wstats = meta["stats"][f"{tag}_{norm}"]
        assert set(stats) == set(wstats)
        for lab, ws in wstats.items():
            if ws is None:
                assert stats[lab] is None
                continue
            for f, w in ws.items():
                g = float(stats[lab][f])
                if norm == "zscore":
                    assert (np.isnan(w) and np.isnan(g)) or abs(g - w) <= SUM_REL * max(abs(w), 1.0), (lab, f)
                else:
                    assert prep_ref.same_bits(g, w), (lab, f)
        if norm == "zscore":
            _close(gn["VALUE_NORMALIZED"], wn["VALUE_NORMALIZED"], 1e-10)
        else:
            assert prep_ref.same_bits(gn["VALUE_NORMALIZED"], wn["VALUE_NORMALIZED"])


def test_remove_outliers_restatement(gold):
    d, meta = gold
    for name, spec in meta["outliers"].items():
        got = prep_ref.remove_outliers(d[f"out_{name}_in"], spec["method"], spec["threshold"])
        assert prep_ref.same_bits(got, d[f"out_{name}_out"]), name


def test_measured_margin_is_recorded(gold):
    _, meta = gold
    assert 0 < meta["sum_rel_dev_max"] < 1e-14                 # a few fp64 ulps: what pandas' own sums deviate by


@pytest.mark.parametrize("kind", ["int", "str"])
def test_edges_from_restated_frames_equal_the_reference_edges(gold, kind):
    d, meta = gold
    labs, cohort = prep_ref.golden_events(d, kind)
    for agg, remove in (("last", True), ("median", False)):
        tag = f"{kind}_{agg}_{'on' if remove else 'off'}"
        want = prep_ref.golden_frame(d, f"{tag}_robust", kind)
        got, _ = prep_ref.normalize(prep_ref.aggregate(labs, cohort, agg, remove, meta["threshold"]), "robust")
        edges = []
        for frame in (got, want):
            pix, lix = graph_build.NodeIndexer(), graph_build.NodeIndexer()
            pix.add_many(cohort["SUBJECT_ID"])
            lix.add_many(frame["ITEMID"])
            edges.append(graph_build.create_patient_lab_edges(frame, pix, lix))
        assert torch.equal(edges[0][0], edges[1][0]) and torch.equal(edges[0][1], edges[1][1])
        assert edges[0][0].shape[1] == len(want) > 0


def test_value_errors_with_the_reference_messages(gold):
    d, _ = gold
    labs, cohort = prep_ref.golden_events(d, "int")
    with pytest.raises(ValueError, match="Unknown aggregation method: first"):
        preprocess.aggregate_lab_values(labs, cohort, method="first")
    with pytest.raises(ValueError, match="Unknown normalization method: l2"):
        preprocess.normalize_lab_values(prep_ref.golden_frame(d, "int_last_on_agg", "int"), method="l2")
    with pytest.raises(ValueError, match="Unknown outlier detection method: mad"):
        preprocess.remove_outliers(np.arange(5.0), method="mad")
    z = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="Unknown aggregation method"):
        preprocess.preprocess_lab_events(z, z, z.double(), z, 4, 2, aggregate="first")
    with pytest.raises(ValueError, match="Unknown normalization method"):
        preprocess.preprocess_lab_events(z, z, z.double(), z, 4, 2, normalize="l2")
    with pytest.raises(ValueError, match="Unknown normalization method"):
        preprocess.LabNormalizer("l2").to_lab_stats()
    assert mmgnn.preprocess_lab_events is preprocess.preprocess_lab_events and mmgnn.LabNormalizer is preprocess.LabNormalizer


def test_ops_refuse_host_tensors():
    from mmgnn import ops
    from mmgnn._lib import MmgError
    z = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(MmgError):
        ops.prep_sort(z, z, z, 4, 2)
    with pytest.raises(ValueError):
        ops.prep_sort(z, z, z, 4, 4096)                       # more labs than MMG_PREP_MAX_LABS
    with pytest.raises(MmgError):
        ops.lab_stats(z, z.double(), 1, 2)


def test_normalizer_tables_and_lab_stats_frame():
    nz = preprocess.LabNormalizer("minmax")
    nz.stats = {"a": {"min": 2.0, "max": 6.0}, "b": None}
    nz.lab_ids = ["a", "b"]
    f = nz.to_lab_stats()
    assert list(f.columns) == ["ITEMID", "mean", "std"] and f["ITEMID"].tolist() == ["a", "b"]
    assert f["mean"].tolist() == [2.0, 0.0] and f["std"].tolist() == [4.0, 1.0]
    assert nz.transform(np.arange(3.0), "b") is not None and nz.inverse_transform(np.arange(3.0), "zz").tolist() == [0.0, 1.0, 2.0]


def test_make_lab_events_shapes_and_determinism():
    ev = make_lab_events(1, seed=3)
    n = ev["patient"].numel()
    assert ev["lab"].shape == ev["value"].shape == ev["time"].shape == (n,)
    assert ev["patient"].dtype == ev["lab"].dtype == ev["time"].dtype == torch.int64 and ev["value"].dtype == torch.float64
    E = ev["edge_index"].shape[1]
    assert (ev["n_patients"], ev["n_labs"], E) == (1834, 50, 61484)
    assert 5.5 * E < n < 6.5 * E
    inside = ev["patient"] < ev["n_patients"]
    assert 0 < int((~inside).sum()) < 0.01 * n
    # exactly the graph's pairs
    code = torch.unique(ev["patient"][inside] * 50 + ev["lab"][inside])
    assert torch.equal(code, torch.sort(ev["edge_index"][0] * 50 + ev["edge_index"][1]).values)
    v = ev["value"]
    assert 1e-4 * n < int((v == 9999.0).sum()) < 3e-3 * n and 2e-3 * n < int(torch.isnan(v).sum()) < 1e-2 * n
    assert int((ev["time"] == torch.iinfo(torch.int64).max).sum()) > 0
    ev2 = make_lab_events(1, seed=3)
    for k in ("patient", "lab", "time"):
        assert torch.equal(ev[k], ev2[k])
    assert prep_ref.same_bits(ev["value"].numpy(), ev2["value"].numpy())
    assert not torch.equal(ev["patient"], make_lab_events(1, seed=4)["patient"])
    labs, cohort = lab_event_frames(ev, string_itemid=True)
    assert list(labs.columns) == ["SUBJECT_ID", "ITEMID", "VALUENUM", "CHARTTIME"] and len(cohort) == 1834
    assert labs["ITEMID"].iloc[0].startswith("lab_") and labs["CHARTTIME"].isna().sum() > 0


def test_c_abi_argument_errors_without_a_gpu():
    from mmgnn import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    nul = ctypes.c_void_p(None)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30
    cnt = ctypes.c_int64(7)
    assert lib.mmg_prep_sort(p, p, p, 0, -1, 4, 2, nul, p, p, nul, p, big, nul) == -1                 # n < 0
    assert lib.mmg_prep_sort(p, p, p, 0, 10, 4, 2049, nul, p, p, nul, p, big, nul) == -1              # too many labs
    assert lib.mmg_prep_sort(p, p, p, 0, 10, 0, 2, nul, p, p, nul, p, big, nul) == -1                 # no patients
    assert lib.mmg_prep_sort(p, p, p, 2, 10, 4, 2, nul, p, p, nul, p, big, nul) == -1                 # key kind
    assert lib.mmg_prep_sort(p, p, p, 0, 10, 4, 2, p, p, p, nul, p, big, nul) == -1                   # value_src alone
    assert lib.mmg_prep_sort(nul, p, p, 0, 10, 4, 2, nul, p, p, nul, p, big, nul) == -1               # null lab
    assert lib.mmg_prep_sort(p, p, p, 0, 10, 4, 2, nul, p, p, nul, p, 64, nul) == -3                  # workspace
    assert b"workspace" in lib.mmg_last_error()
    assert lib.mmg_prep_sort(p, p, p, 0, 0, 4, 2, nul, p, p, nul, p, big, nul) == 0                   # n = 0 is valid
    assert lib.mmg_prep_sort_ws_bytes(1000) > 1000 * 24
    assert lib.mmg_lab_stats(p, p, 10, 4, 0, p, p, big, nul) == -1                                    # n_labs = 0
    assert lib.mmg_lab_stats(p, p, 10, 4, 2, nul, p, big, nul) == -1                                  # null stats
    assert lib.mmg_lab_stats(p, p, 10, 4, 2, p, p, 8, nul) == -3
    assert lib.mmg_lab_quantiles(p, p, -5, 1, 2, p, p, big, nul) == -1
    assert lib.mmg_lab_quantiles(p, nul, 5, 1, 2, p, p, big, nul) == -1
    assert lib.mmg_lab_quantiles(p, p, 5, 1, 2, p, nul, 0, nul) == -3
    assert lib.mmg_lab_stats_ws_bytes(50) > 0 and lib.mmg_lab_quantiles_ws_bytes(50) > 0
    agg = lib.mmg_lab_aggregate
    assert agg(p, p, 10, 4, 2, 5, 0, 5.0, nul, p, p, p, ctypes.byref(cnt), p, big, nul) == -1         # method
    assert agg(p, p, 10, 4, 2, 0, 3, 5.0, p, p, p, p, ctypes.byref(cnt), p, big, nul) == -1           # outlier method
    assert agg(p, p, 10, 4, 2, 0, 1, 5.0, nul, p, p, p, ctypes.byref(cnt), p, big, nul) == -1         # removal, no table
    assert agg(p, p, 10, 4, 2, 0, 0, 5.0, nul, p, p, p, None, p, big, nul) == -1                      # no count
    assert agg(p, p, 10, 4, 2, 0, 0, 5.0, nul, p, p, p, ctypes.byref(cnt), p, 16, nul) == -3
    assert agg(p, p, 0, 4, 2, 0, 0, 5.0, nul, p, p, p, ctypes.byref(cnt), p, big, nul) == 0 and cnt.value == 0
    assert lib.mmg_lab_aggregate_ws_bytes(1000) > 1000 * 16
    assert lib.mmg_lab_transform(3, 0, 0.0, p, p, 10, 2, p, p, nul) == -1                             # mode
    assert lib.mmg_lab_transform(0, 0, 5.0, p, p, 10, 2, p, p, nul) == -1                             # outlier "none"
    assert lib.mmg_lab_transform(1, 3, 0.0, p, p, 10, 2, p, p, nul) == -1                             # normalisation
    assert lib.mmg_lab_transform(1, 0, 0.0, p, p, 10, 2, nul, p, nul) == -1                           # null table
    assert lib.mmg_lab_transform(1, 0, 0.0, p, p, 0, 2, p, p, nul) == 0
    assert lib.mmg_lab_inverse_matrix(0, p, 10, 8, 4, p, p, 8, nul) == -1                             # ld < n_labs
    assert lib.mmg_lab_inverse_matrix(5, p, 10, 8, 8, p, p, 8, nul) == -1
    assert lib.mmg_lab_inverse_matrix(0, p, 10, 8, 8, p, nul, 8, nul) == -1
    assert lib.mmg_lab_inverse_matrix(0, p, 0, 8, 8, p, p, 8, nul) == 0
