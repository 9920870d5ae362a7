"""Split-conformal intervals on the host (mmgnn/conformal.py): the numpy path EQUALS the loop reference of
conformal_ref.py, the defining rank property holds as an integer identity, the coverage on seeded synthetic data lies
inside its derived bound, and the plumbing around it (state dict, inference dicts, the derived binding)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import conformal as cf
from mmgnn import inference
import conformal_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
EDGES3 = [0.0, 6.0, 16.0, float("inf")]
ALPHAS = [0.05, 0.1, 0.2, 0.5]


def same(a, b):
    """equal as values: the same NaN positions, the same infinities, equal numbers (-0 == +0)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def host_fit(c, edges, alpha, mode, min_count=0):
    return cf.host_fit(c["pred"], c["target"], c["patient"], c["lab"], c["n_labs"], c["deg"], edges, alpha, mode, min_count)


def ref_fit(c, edges, alpha, mode, min_count=0):
    return ref.fit(c["pred"], c["target"], c["patient"], c["lab"], c["n_labs"], c["deg"], edges, alpha, mode, min_count)


@pytest.mark.parametrize("mode", ["signed", "absolute"])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_host_tables_bounds_and_counts_equal_the_reference(mode, alpha):
    c = ref.make_case()
    edges = [1.0, 6.0, 16.0, float("inf")]                   # degree 0 lies in no bin
    got, want = host_fit(c, edges, alpha, mode), ref_fit(c, edges, alpha, mode)
    for g, w, name in zip(got, want, ("table", "level", "n_used", "dropped")):
        assert same(g, w), name
    assert got[3].tolist()[0] == 4 and got[3].tolist()[1] == 3 and got[3][2] > 0 and got[3][3] >= 3
    assert set(got[1].tolist()) >= {0, 2}                    # the empty lab and the one-pair lab fall back to all pairs
    table = got[0]
    for shift in (False, True):
        a = cf.host_apply_pairs(c["pred"], c["patient"], c["lab"], c["n_labs"], c["deg"], edges, table, shift)
        b = ref.apply_pairs(c["pred"], c["patient"], c["lab"], c["n_labs"], c["deg"], edges, table, shift)
        for x, y in zip(a, b):
            assert same(x, y)
    counts, width = cf.host_coverage(c["pred"], c["target"], c["patient"], c["lab"], c["n_labs"], c["deg"], edges, table)
    rc, rw = ref.coverage(c["pred"], c["target"], c["patient"], c["lab"], c["n_labs"], c["deg"], edges, table)
    assert same(counts, rc)
    assert counts[:, 0].sum() + counts[:, 5].sum() == c["pred"].size
    for cell, ws in enumerate(rw):
        tot = math.fsum(float(w) for w in ws)
        assert abs(width[cell] - tot) <= (len(ws) + 8) * 2.0 ** -53 * math.fsum(abs(float(w)) for w in ws)


@pytest.mark.parametrize("mode", ["signed", "absolute"])
def test_min_count_forces_every_fallback_level(mode):
    c = ref.make_case(special=False, n=600)
    seen = set()
    for mc in (0, 30, 150, 450, 10 ** 6):
        got, want = host_fit(c, EDGES3, 0.1, mode, mc), ref_fit(c, EDGES3, 0.1, mode, mc)
        for g, w in zip(got, want):
            assert same(g, w)
        seen |= set(got[1].tolist())
        if mc == 10 ** 6:
            assert set(got[1].tolist()) == {3} and np.all(np.isneginf(got[0][0])) and np.all(np.isposinf(got[0][1]))
            assert not got[0][2].any() and not got[2].any()
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("mode", ["signed", "absolute"])
def test_no_pairs_gives_an_all_unusable_table(mode):
    z = np.zeros(0)
    c = dict(pred=z.astype(F32), target=z.astype(F32), patient=z.astype(np.int64), lab=z.astype(np.int64), n_labs=3,
             deg=np.array([1, 7], np.int32))
    got, want = host_fit(c, EDGES3, 0.1, mode), ref_fit(c, EDGES3, 0.1, mode)
    for g, w in zip(got, want):
        assert same(g, w)
    assert set(got[1].tolist()) == {3} and got[3].tolist() == [0, 0, 0, 0]
    obj = cf.LabConformal(score=mode).fit(c["pred"], c["target"], c["lab"], c["patient"], c["deg"], n_labs=3)
    p, lo, hi = obj.predict(np.array([1.5], F32), np.array([0]), np.array([1]))
    assert p[0] == F32(1.5) and lo[0] == -np.inf and hi[0] == np.inf


@pytest.mark.parametrize("mode", ["signed", "absolute"])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_segment_statistics_equal_the_reference(mode, alpha):
    rng = np.random.default_rng(5)
    n, n_seg = 3000, 40
    keys = rng.standard_normal(n).astype(F32)
    keys[::7] = F32(0.5)
    keys[1:50:5] = [np.inf, -np.inf, np.nan, 0.0, -0.0] * 2
    seg = rng.integers(0, n_seg + 1, n).astype(np.int32)     # n_seg: ignored
    seg[seg == 3] = 4                                        # an empty segment
    seg[seg == 9] = 8
    seg[5] = 9                                               # a segment of one key
    keys[5] = 2.0
    for mc in (0, 80):
        got = cf.host_seg_order_stats(keys, seg, n_seg, alpha, mode, mc)
        want = ref.seg_order_stats(keys, seg, n_seg, alpha, mode, mc)
        for g, w, name in zip(got, want, ("count", "q_lo", "q_hi", "shift", "usable")):
            assert same(g, w), name
        assert got[0][3] == 0 and got[0][9] == 1 and not got[4][3]


@pytest.mark.parametrize("mode", ["signed", "absolute"])
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("ties", [False, True])
def test_a_usable_segment_covers_exactly_its_ranks_of_its_own_pairs(mode, alpha, ties):
    """The defining property: of its m own calibration keys a usable segment's bounds cover k_hi - k_lo + 1 (signed) or
    k_hi (absolute) -- exactly with distinct keys, at least with ties."""
    rng = np.random.default_rng(11)
    n, n_seg = 4000, 25
    seg = rng.integers(0, n_seg, n).astype(np.int32)
    seg[seg == 0] = 1
    seg[:3] = 0                                              # three keys: unusable at small alpha
    keys = ((rng.permutation(n) + 1) * rng.choice([-1, 1], n)).astype(F32)      # distinct, and distinct in |.|
    if ties:
        keys = np.round(keys / 40)
    if mode == "absolute":
        keys = np.abs(keys)                                  # the primitive takes the keys as they are
    count, q_lo, q_hi, _, usable = cf.host_seg_order_stats(keys, seg, n_seg, alpha, mode)
    assert usable.sum() >= n_seg - 1
    for s in range(n_seg):
        if not usable[s]:
            continue
        k = keys[seg == s]
        k_lo, k_hi = ref.ranks(int(count[s]), alpha, mode)
        covered = int(((k >= q_lo[s]) & (k <= q_hi[s])).sum())
        want = k_hi - k_lo + 1 if mode == "signed" else k_hi
        if ties:
            assert covered >= want
        else:
            assert covered == want
    if not ties and mode == "signed":
        assert int(usable.sum()) > 0


@pytest.mark.parametrize("mode", ["signed", "absolute"])
def test_coverage_on_synthetic_data_lies_inside_its_derived_bound(mode):
    """Per cell and overall |coverage - (1 - alpha)| <= 5 sqrt(alpha (1 - alpha) (1 / (m + 2) + 1 / n_eval)): the coverage
    given the calibration set is Beta(k, m + 1 - k), the evaluation count is binomial on top."""
    alpha, m, n_eval = 0.1, 400, 1000
    edges, deg, cal, ev = ref.synthetic(3, m, n_eval)
    obj = cf.LabConformal(alpha=alpha, score=mode, bins=edges, labels=("a", "b", "c", "d"))
    obj.fit(cal[0], cal[1], cal[2], cal[3], deg, n_labs=12)
    assert set(obj.level.tolist()) == {0} and set(obj.n_used.tolist()) == {m}
    counts, _ = obj.coverage_counts(ev[0], ev[1], ev[2], ev[3])
    assert counts[:-1, 0].tolist() == [n_eval] * 48 and not counts[:, 4:].any()
    worst = 0.0
    for c in range(48):
        d = abs(counts[c, 1] / n_eval - (1 - alpha))
        worst = max(worst, d / ref.coverage_bound(alpha, m, n_eval, 1.0))
        assert d <= ref.coverage_bound(alpha, m, n_eval), (c, d)
    overall = counts[:-1, 1].sum() / counts[:-1, 0].sum()
    # overall: every cell has its own Beta draw, so the calibration term shrinks with the cells too; the bound with the
    # cell's m and all evaluation pairs is the wider, safe one
    print(f"{mode}: worst cell {worst:.2f} sd, overall {overall:.4f}")
    assert abs(overall - (1 - alpha)) <= ref.coverage_bound(alpha, m, 48 * n_eval)
    frame = obj.coverage(ev[0], ev[1], ev[2], ev[3])
    assert list(frame.columns) == cf.COVERAGE_COLUMNS and len(frame) == 1 + 12 + 4
    assert frame.iloc[0]["n"] == 48 * n_eval and frame.iloc[0]["coverage"] == overall
    assert frame[frame.scope == "lab"]["n"].tolist() == [4 * n_eval] * 12


def test_state_dict_round_trip_and_table_frame():
    c = ref.make_case()
    a = cf.LabConformal(alpha=0.2, score="signed", min_count=20, point="median")
    a.fit(c["pred"], c["target"], c["lab"], c["patient"], c["deg"], n_labs=c["n_labs"])
    state = a.state_dict()
    b = cf.LabConformal().load_state_dict(state)
    assert (b.alpha, b.score, b.point, b.min_count, b.n_labs, b.edges, b.labels) == \
        (a.alpha, a.score, a.point, a.min_count, a.n_labs, a.edges, a.labels)
    for x, y in zip(a._host, b._host):
        assert same(x, y)
    for x, y in zip(a.predict(c["pred"], c["lab"], c["patient"]), b.predict(c["pred"], c["lab"], c["patient"])):
        assert same(x, y)
    m = c["pred"][:20].reshape(4, 5)
    rows = np.array([3, 3, 0, 39])
    pm = a.predict_matrix(m, rows)
    pp = a.predict(m.reshape(-1), np.tile(np.arange(5), 4), rows.repeat(5))
    for x, y in zip(pm, pp):
        assert same(x.reshape(-1), y)
    assert not same(pm[0], m)                                # point="median" moves the point
    frame = a.table_frame({0: "glucose"})
    assert list(frame.columns) == cf.TABLE_COLUMNS and len(frame) == 15
    assert frame.lab_name[0] == "glucose" and frame.lab_name[3] == "Lab_1" and frame.degree_bin.tolist()[:3] == ["0-5", "6-15", "16+"]
    assert set(frame.level) <= set(cf.LEVELS)
    with pytest.raises(ValueError):
        cf.LabConformal(alpha=1.0)
    with pytest.raises(ValueError):
        cf.LabConformal(score="absolute", point="median")
    with pytest.raises(RuntimeError):
        cf.LabConformal().predict(c["pred"], c["lab"], c["patient"])


def test_inference_dicts_gain_exactly_the_four_interval_keys():
    lab_indexer = {"A": 0, "B": 1, "C": 2}
    lab_stats = pd.DataFrame({"ITEMID": ["A", "B", "C"], "mean": [10.0, 20.0, 30.0], "std": [2.0, 4.0, 8.0]})
    pred = np.array([0.5, -1.0, 0.25], F32)
    args = (pred, np.array([0, 1]), np.array([0.4, -0.9], F32), np.array([True, False]), lab_stats, lab_indexer)
    plain = inference.lab_report(*args)
    assert set(plain["masked_labs"]["A"]) == {"predicted", "actual", "error", "normalized_predicted", "normalized_actual"}
    assert set(plain["truly_missing_labs"]["C"]) == {"predicted", "normalized_predicted", "note"}
    lower, upper = pred - F32(0.5), pred + F32(1.0)
    with_iv = inference.lab_report(*args, bounds=(lower, upper))
    extra = {"lower", "upper", "normalized_lower", "normalized_upper"}
    assert with_iv["measured_labs"] == plain["measured_labs"]
    for group, name, idx in (("masked_labs", "A", 0), ("truly_missing_labs", "C", 2)):
        got, base = with_iv[group][name], plain[group][name]
        assert set(got) == set(base) | extra and {k: got[k] for k in base} == base
        st = lab_stats.iloc[idx]
        assert got["normalized_lower"] == float(lower[idx]) and got["normalized_upper"] == float(upper[idx])
        assert got["lower"] == float(lower[idx] * st["std"] + st["mean"]) and got["upper"] == float(upper[idx] * st["std"] + st["mean"])
        assert got["lower"] <= got["predicted"] <= got["upper"]
    import inspect
    for fn in (inference.predict_for_patients, inference.predict_for_patient):
        assert inspect.signature(fn).parameters["intervals"].default is None


def test_binding_is_derived_from_the_header_and_matches_the_library():
    from mmgnn import conformal_ops as co
    calls = {"mmg_seg_order_stats", "mmg_cf_fit", "mmg_cf_apply_pairs", "mmg_cf_apply_matrix", "mmg_cf_coverage"}
    with_ws = calls - {"mmg_cf_apply_pairs", "mmg_cf_apply_matrix"}
    assert set(co.SIGNATURES) == calls | {c + "_ws_bytes" for c in with_ws}
    for name in with_ws:
        assert [p[0] for p in co.PARAMS[name]][-3:] == ["ws", "ws_bytes", "stream"], name
    for name in calls - with_ws:
        assert [p[0] for p in co.PARAMS[name]][-1] == "stream" and "ws" not in [p[0] for p in co.PARAMS[name]]
    assert (co.CF_MAX_LABS, co.CF_MAX_CELLS, co.CF_DROP_KINDS, co.CF_COV_FIELDS) == (2048, 32768, 4, 6)
    from mmgnn import _lib
    assert co.CF_MAX_BINS == _lib.MMG_AN_MAX_BINS
    assert len(cf.DROP_KINDS) == co.CF_DROP_KINDS and len(cf.COV_FIELDS) == co.CF_COV_FIELDS
    assert os.path.exists(co.LIB_PATH), "libmmgnn_conformal.so is not built (make -C multi-modal-gnn_amd/csrc)"
    nm = next((c for c in ("nm", "llvm-nm", "/opt/rocm/llvm/bin/llvm-nm") if shutil.which(c)), None)
    assert nm is not None, "no nm found (nm, llvm-nm, /opt/rocm/llvm/bin/llvm-nm)"
    out = subprocess.run([nm, "-D", "--defined-only", co.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {s for s in exported if s.startswith("mmg_")} == set(co.SIGNATURES)
