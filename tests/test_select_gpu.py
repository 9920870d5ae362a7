"""Feature-space selection on the device (csrc/select.hip through mmgnn.preprocess) against the reference's stored
frames (tests/golden/select_small.npz) and, on seeded random tensors and the synthetic tables, against the restatement
select_ref.py.  All the work is integer or text: every comparison is exact equality, there is no tolerance anywhere."""
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import _lib, graph_build, ops, preprocess
from mmgnn.synth import code_event_frames, lab_event_frames, make_code_events, make_lab_events
import prep_ref
import select_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "select_small.npz")
TILE = 1024                    # RADIX_TILE of csrc/radix_sort.h (checked below)
I64 = np.iinfo(np.int64)


def test_tile_size_is_the_sort_s():
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "radix_sort.h")).read()
    assert f"constexpr int RADIX_TILE = {TILE};" in src


@pytest.fixture(scope="module")
def gold():
    d = np.load(GOLDEN)
    meta = json.loads(str(d["__meta__"]))
    return d, meta, select_ref.unpack_frame(d, meta, "cohort")


# ------------------------------------------------------------------------------------------ the reference's frames
@pytest.mark.parametrize("kind", ["int", "str"])
def test_filter_labs_matches_the_reference(gold, kind):
    d, meta, cohort = gold
    labs = select_ref.unpack_frame(d, meta, f"{kind}/labevents")
    items = select_ref.unpack_frame(d, meta, f"{kind}/d_labitems")
    for k in meta["cases"]["labs"]:
        got, sel = preprocess.filter_labs_for_cohort(labs, cohort, items, top_k=k, min_patient_count=meta["min"]["labs"])
        assert select_ref.same_frame(got, select_ref.unpack_frame(d, meta, f"{kind}/labs_top{k}")), k
        assert select_ref.same_frame(sel, select_ref.unpack_frame(d, meta, f"{kind}/labitems_top{k}")), k


def test_process_diagnoses_matches_the_reference(gold):
    d, meta, cohort = gold
    dx = select_ref.unpack_frame(d, meta, "dx/in")
    for collapse, k in meta["cases"]["dx"]:
        got = preprocess.process_diagnoses(dx, cohort, collapse_to_3digit=collapse, top_k=k, min_patient_count=meta["min"]["dx"])
        assert select_ref.same_frame(got, select_ref.unpack_frame(d, meta, f"dx/out_{int(collapse)}_top{k}")), (collapse, k)
    bare = preprocess.process_diagnoses(dx[["SUBJECT_ID", "HADM_ID", "ICD9_CODE"]], cohort, min_patient_count=meta["min"]["dx"])
    assert select_ref.same_frame(bare, select_ref.unpack_frame(d, meta, "dx/out_bare"))


def test_process_medications_matches_the_reference(gold):
    d, meta, cohort = gold
    rx = select_ref.unpack_frame(d, meta, "rx/in")
    for norm, k in meta["cases"]["rx"]:
        got = preprocess.process_medications(rx, cohort, normalize_names=norm, top_k=k, min_patient_count=meta["min"]["rx"])
        assert select_ref.same_frame(got, select_ref.unpack_frame(d, meta, f"rx/out_{int(norm)}_top{k}")), (norm, k)


# ------------------------------------------------------------------------------------------ select_codes
def _device_select(patient, code, n_patients, n_codes, valid, min_count, top_k, rows):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    out = preprocess.select_codes(t(patient), t(code), n_patients, n_codes, valid=None if valid is None else t(valid),
                                  min_patient_count=min_count, top_k=top_k, rows=rows)
    assert [o.dtype for o in out] == [torch.int64, torch.int64, torch.int32, torch.uint8, torch.int32]
    return [o.cpu().numpy() for o in out]


def _check(patient, code, n_patients, n_codes, valid=None, min_count=2, top_k=None):
    """Both row modes against the restatement, + the properties of out_rows."""
    res = {}
    for rows in ("all", "first"):
        got = _device_select(patient, code, n_patients, n_codes, valid, min_count, top_k, rows)
        want = select_ref.select_codes(patient, code, n_patients, n_codes, valid, min_count, top_k, rows)
        for g, w, name in zip(got, want, ("n_patients_per_code", "n_rows_per_code", "rank", "selected", "out_rows")):
            assert g.shape == w.shape and np.array_equal(g, w), (rows, name)
        out = got[4].astype(np.int64)
        assert np.all(np.diff(out) > 0)                        # strictly ascending
        if rows == "first" and len(out):
            key = code[out] * np.int64(n_patients) + patient[out]
            assert len(np.unique(key)) == len(key)             # one row per pair ...
            ok = (code >= 0) & (code < n_codes) & (patient >= 0) & (patient < n_patients) & (True if valid is None else valid != 0)
            idx = np.flatnonzero(ok)
            allkey = code[idx] * np.int64(n_patients) + patient[idx]
            order = np.argsort(allkey, kind="stable")
            heads = np.r_[True, allkey[order][1:] != allkey[order][:-1]]
            smallest = dict(zip(allkey[order][heads].tolist(), idx[order][heads].tolist()))
            assert all(smallest[k] == r for k, r in zip(key.tolist(), out.tolist()))      # ... the smallest index
        res[rows] = got
    return res


def _random(n, n_patients, n_codes, seed, junk=True, live_codes=None):
    rng = np.random.default_rng(seed)
    live = np.sort(rng.choice(n_codes, size=live_codes or max(1, n_codes // 2), replace=False))   # codes without a row exist
    w = 1.0 / np.arange(1, len(live) + 1)
    code = live[rng.choice(len(live), size=n, p=w / w.sum())].astype(np.int64)
    patient = rng.integers(0, min(n_patients, max(4, n // 3 + 1)), n).astype(np.int64)
    valid = (rng.random(n) < 0.9).astype(np.uint8)
    if junk and n >= 8:
        bad = rng.choice(n, size=max(2, n // 50), replace=False)
        code[bad[::2]] = rng.choice([-1, n_codes, I64.min, I64.max], size=len(bad[::2]))
        patient[bad[1::2]] = rng.choice([-1, n_patients, I64.min, I64.max], size=len(bad[1::2]))
    return patient, code, valid


@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_select_codes_around_the_sort_tile(n):
    patient, code, valid = _random(n, 37, 23, seed=100 + n)
    _check(patient, code, 37, 23, None, min_count=1 if n < 2 else 3, top_k=None)
    _check(patient, code, 37, 23, valid, min_count=1 if n < 2 else 3, top_k=4)


def test_select_codes_more_codes_than_the_lab_kernels_take():
    n, n_patients, n_codes = 200_003, 1834, 5000
    assert n_codes > ops.PREP_MAX_LABS
    patient, code, valid = _random(n, n_patients, n_codes, seed=7)
    r = _check(patient, code, n_patients, n_codes, valid, min_count=5, top_k=64)
    n_pat, n_rows, rank, sel, _ = r["all"]
    assert int((n_rows == 0).sum()) >= n_codes // 2 and int(sel.sum()) == 64 and int((rank >= 0).sum()) > 64
    assert len(r["first"][4]) < len(r["all"][4])               # repeated pairs
    eligible = int((rank >= 0).sum())
    for k in (0, eligible, eligible + 5):                      # no code, exactly every eligible one, more than there are
        got = _check(patient, code, n_patients, n_codes, valid, min_count=5, top_k=k)["all"]
        assert int(got[3].sum()) == min(k, eligible)
    assert len(_device_select(patient, code, n_patients, n_codes, valid, 5, 0, "all")[4]) == 0


def test_select_codes_keys_beyond_32_bits():
    n, n_patients, n_codes = 6001, 2 ** 20 + 3, 5000
    assert (n_codes - 1) * n_patients > 2 ** 32
    rng = np.random.default_rng(11)
    code = rng.choice([0, 1, 17, 2048, 4095, 4096, 4998, 4999], size=n).astype(np.int64)
    patient = rng.choice(np.r_[0, 1, 2 ** 16, 2 ** 20, 2 ** 20 + 2, rng.integers(0, n_patients, 40)], size=n).astype(np.int64)
    r = _check(patient, code, n_patients, n_codes, None, min_count=3, top_k=5)
    assert int(r["all"][3].sum()) == 5 and r["all"][0][4999] > 0 and r["all"][0][4998] > 0


def test_select_codes_nothing_counted_or_nothing_eligible():
    patient, code, _ = _random(3000, 50, 40, seed=3, junk=False)
    for p, c, v in ((patient, code, np.zeros(3000, np.uint8)), (patient + 50, code, None), (patient, code - 40, None)):
        for rows in ("all", "first"):
            n_pat, n_rows, rank, sel, out = _device_select(p, c, 50, 40, v, 0, None, rows)      # every row is ignored
            assert not n_pat.any() and not n_rows.any() and np.all(rank == -1) and not sel.any() and len(out) == 0
    r = _check(patient, code, 50, 40, None, min_count=51, top_k=None)                          # more than there are patients
    for rows in ("all", "first"):
        n_pat, n_rows, rank, sel, out = r[rows]
        assert n_rows.sum() == 3000 and n_pat.max() <= 50 and np.all(rank == -1) and not sel.any() and len(out) == 0


def test_select_codes_tie_across_the_cut():
    # codes 9, 3, 6, 1 with 4 patients each, code 5 with 7, code 2 with 3; the rows of the later codes come first
    plan = [(9, 4), (6, 4), (3, 4), (1, 4), (5, 7), (2, 3)]
    patient = np.concatenate([np.repeat(np.arange(k), 2) for _, k in plan]).astype(np.int64)
    code = np.concatenate([np.full(2 * k, c) for c, k in plan]).astype(np.int64)
    for rows in ("all", "first"):
        n_pat, _, rank, sel, out = _device_select(patient, code, 8, 12, None, 3, 3, rows)
        assert rank[[5, 1, 3, 6, 9, 2]].tolist() == [0, 1, 2, 3, 4, 5] and int((rank >= 0).sum()) == 6
        assert np.flatnonzero(sel).tolist() == [1, 3, 5]       # 5 by count, then the two SMALLER of the four tied codes
        assert set(code[out]) == {1, 3, 5} and len(out) == (30 if rows == "all" else 15)
    _check(patient, code, 8, 12, None, min_count=3, top_k=3)


def test_select_codes_ignores_out_of_range_rows():
    patient, code, valid = _random(5000, 64, 300, seed=5, junk=False)
    base = _device_select(patient, code, 64, 300, valid, 2, 20, "first")
    rng = np.random.default_rng(6)
    junk_p = np.array([-1, 64, I64.min, I64.max, 3, 3, 3, 3, -1, I64.max], np.int64)
    junk_c = np.array([3, 3, 3, 3, -1, 300, I64.min, I64.max, -1, I64.max], np.int64)
    at = np.sort(rng.choice(5000, size=len(junk_p), replace=False)) + np.arange(len(junk_p))     # insertion points
    keep = np.ones(5000 + len(at), bool)
    keep[at] = False
    p2, c2, v2 = (np.empty(len(keep), a.dtype) for a in (patient, code, valid))
    p2[keep], c2[keep], v2[keep] = patient, code, valid
    p2[at], c2[at], v2[at] = junk_p, junk_c, 1
    for rows in ("all", "first"):
        base = _device_select(patient, code, 64, 300, valid, 2, 20, rows)
        got = _device_select(p2, c2, 64, 300, v2, 2, 20, rows)
        for g, w in zip(got[:4], base[:4]):
            assert np.array_equal(g, w)
        assert np.array_equal(np.flatnonzero(keep)[base[4]], got[4])        # the same rows, renumbered
    _check(p2, c2, 64, 300, v2, min_count=2, top_k=20)


def test_select_codes_is_stateless_and_reproducible():
    n, n_patients, n_codes = 40_000, 700, 3000
    patient, code, valid = _random(n, n_patients, n_codes, seed=9)
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    tp, tc, tv = t(patient), t(code), t(valid)
    lib = _lib.load()
    for rows in ("all", "first"):
        call = lambda: preprocess.select_codes(tp, tc, n_patients, n_codes, valid=tv, min_patient_count=3, top_k=50, rows=rows)   # noqa: E731
        first = call()
        ws = ops.workspace(lib.mmg_code_select_ws_bytes(n, n_codes), torch.device(DEV))
        ws.fill_(0xFF)                                         # whatever an earlier call left behind
        second = call()
        ws.zero_()
        third = call()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fourth = call()
        side.synchronize()
        for other in (second, third, fourth):
            assert all(torch.equal(a, b) for a, b in zip(first, other))
        want = select_ref.select_codes(patient, code, n_patients, n_codes, valid, 3, 50, rows)
        assert all(np.array_equal(a.cpu().numpy(), w) for a, w in zip(first, want))


# ------------------------------------------------------------------------------------------ raw frames -> graph
CONFIG = {"feature_space": {"labs": {"top_k": 30, "min_patient_count": 10, "aggregate": "last", "normalize": "zscore",
                                     "outlier_std_threshold": 5.0},
                            "diagnoses": {"collapse_to_3digit": True, "top_k": 60, "min_patient_count": 5},
                            "medications": {"normalize_names": True, "top_k": 80}},
          "graph": {"edge_types": {k: {"enabled": True, "bidirectional": True}
                                   for k in ("patient_lab", "patient_diagnosis", "patient_medication")}}}


def test_preprocess_frames_equals_the_restated_chain_and_builds_the_graph():
    cap = 50_000
    ev = make_lab_events(1, seed=2)
    labs, _ = lab_event_frames(ev, string_itemid=True)
    labs = labs.iloc[:cap]
    dx, cohort = code_event_frames(make_code_events(1, seed=2, kind="diagnosis"), "diagnosis")
    rx, _ = code_event_frames(make_code_events(1, seed=2, kind="medication"), "medication")
    dx, rx = dx.iloc[:cap], rx.iloc[:cap]
    assert dx["ICD9_CODE"].nunique() > ops.PREP_MAX_LABS or rx["DRUG"].nunique() > ops.PREP_MAX_LABS
    items = pd.DataFrame({"ITEMID": [f"lab_{i:03d}" for i in range(ev["n_labs"])][::-1], "LABEL": [f"L{i}" for i in range(ev["n_labs"])]})
    got = preprocess.preprocess_frames(labs, items, dx, rx, cohort, CONFIG)
    assert sorted(got) == ["diagnoses", "lab_normalizer", "labitems", "labs", "medications"]

    w_labs, w_items, w_dx, w_rx = select_ref.frames(labs, items, dx, rx, cohort, CONFIG)
    assert select_ref.same_frame(got["labitems"], w_items) and len(w_items) == 30
    assert select_ref.same_frame(got["diagnoses"], w_dx) and select_ref.same_frame(got["medications"], w_rx)
    w_norm, w_stats = prep_ref.normalize(prep_ref.aggregate(w_labs, cohort, "last", True, 5.0), "zscore")
    g_norm = got["labs"]
    assert list(g_norm.columns) == list(w_norm.columns) and len(g_norm) == len(w_norm)
    assert np.array_equal(g_norm["SUBJECT_ID"].to_numpy(), w_norm["SUBJECT_ID"].to_numpy())      # row for row
    assert g_norm["ITEMID"].tolist() == w_norm["ITEMID"].tolist()
    # "last" picks one of the event values: bit-equal (the z-scores are sums; test_prep_gpu.py holds them to their bound)
    assert prep_ref.same_bits(g_norm["VALUE"], w_norm["VALUE"])
    assert set(got["lab_normalizer"].stats) == set(w_stats)

    g = graph_build.build_heterogeneous_graph(cohort, got["labs"], got["diagnoses"], got["medications"], None,
                                              got["labitems"], CONFIG)
    assert g["patient"].num_nodes == len(cohort)
    assert g["lab"].num_nodes == len(got["labitems"]) == 30
    assert g["diagnosis"].num_nodes == got["diagnoses"]["ICD3_CODE"].nunique() == 60
    assert g["medication"].num_nodes == got["medications"]["DRUG"].nunique() > 20
    assert g["patient", "has_diagnosis", "diagnosis"].edge_index.shape[1] == len(got["diagnoses"])
    assert g["patient", "has_medication", "medication"].edge_index.shape[1] == len(got["medications"])
    assert len(g["lab"].metadata) == 30
