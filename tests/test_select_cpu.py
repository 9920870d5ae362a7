"""Feature-space selection on the host: the numpy / pandas restatement (select_ref.py) against what the reference's own
filter_labs_for_cohort / process_diagnoses / process_medications / normalize_drug_name returned
(tests/golden/select_small.npz), the drug-name rules, the exported symbols, the C-ABI argument checks of
mmg_code_select, the refusals of the Python layer and the code-event generator.  Everything is integer or text: exact."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import preprocess
from mmgnn.synth import code_event_frames, make_code_events
import select_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "select_small.npz")


@pytest.fixture(scope="module")
def gold():
    d = np.load(GOLDEN)
    return d, json.loads(str(d["__meta__"]))


@pytest.mark.parametrize("kind", ["int", "str"])
def test_lab_restatement_matches_the_reference(gold, kind):
    d, meta = gold
    cohort = select_ref.unpack_frame(d, meta, "cohort")
    labs = select_ref.unpack_frame(d, meta, f"{kind}/labevents")
    items = select_ref.unpack_frame(d, meta, f"{kind}/d_labitems")
    for k in meta["cases"]["labs"]:
        got, sel = select_ref.filter_labs(labs, cohort, items, k, meta["min"]["labs"])
        assert select_ref.same_frame(got, select_ref.unpack_frame(d, meta, f"{kind}/labs_top{k}")), k
        assert select_ref.same_frame(sel, select_ref.unpack_frame(d, meta, f"{kind}/labitems_top{k}")), k
        assert len(sel) == (k if k is not None else 11)


def test_diagnosis_restatement_matches_the_reference(gold):
    d, meta = gold
    cohort, dx = select_ref.unpack_frame(d, meta, "cohort"), select_ref.unpack_frame(d, meta, "dx/in")
    for collapse, k in meta["cases"]["dx"]:
        want = select_ref.unpack_frame(d, meta, f"dx/out_{int(collapse)}_top{k}")
        assert select_ref.same_frame(select_ref.diagnoses(dx, cohort, collapse, k, meta["min"]["dx"]), want), (collapse, k)
        assert ("ICD3_CODE" in want.columns) == collapse and ("ICD9_CODE" in want.columns) != collapse
    bare = select_ref.diagnoses(dx[["SUBJECT_ID", "HADM_ID", "ICD9_CODE"]], cohort, True, None, meta["min"]["dx"])
    assert select_ref.same_frame(bare, select_ref.unpack_frame(d, meta, "dx/out_bare"))
    assert list(bare.columns) == ["SUBJECT_ID", "ICD3_CODE"] and "nan" in set(bare["ICD3_CODE"])


def test_medication_restatement_matches_the_reference(gold):
    d, meta = gold
    cohort, rx = select_ref.unpack_frame(d, meta, "cohort"), select_ref.unpack_frame(d, meta, "rx/in")
    for norm, k in meta["cases"]["rx"]:
        want = select_ref.unpack_frame(d, meta, f"rx/out_{int(norm)}_top{k}")
        assert select_ref.same_frame(select_ref.medications(rx, cohort, norm, k, meta["min"]["rx"]), want), (norm, k)
        assert list(want.columns) == ["SUBJECT_ID", "DRUG", "ROUTE", "PRN"]


def test_normalize_drug_name_matches_the_reference(gold):
    d, meta = gold
    raw, want = d["drug/raw"].tolist(), d["drug/normalized"].tolist()
    assert len(raw) > 30 and "" in want
    for fn in (preprocess.normalize_drug_name, select_ref.drug_name):
        assert [fn(r) for r in raw] == want
        assert [fn(np.nan), fn(None)] == meta["drug_missing"] == ["", ""]
    assert mmgnn.normalize_drug_name is preprocess.normalize_drug_name and mmgnn.select_codes is preprocess.select_codes


def test_restated_select_codes_on_a_hand_made_table():
    #        row: 0  1  2  3  4  5  6  7  8  9
    patient = [0, 0, 1, 2, 2, 9, 1, 0, 3, 1]
    code = [1, 1, 1, 0, 0, 1, 3, 3, 7, 0]                      # patient 9 and code 7 are out of range (4 patients, 4 codes)
    n_pat, n_rows, rank, sel, rows = select_ref.select_codes(patient, code, 4, 4, None, 2, 1, "first")
    assert n_pat.tolist() == [2, 2, 0, 2] and n_rows.tolist() == [3, 3, 0, 2]
    assert rank.tolist() == [0, 1, -1, 2] and sel.tolist() == [1, 0, 0, 0]      # three-way tie: the smallest code
    assert rows.tolist() == [3, 9]
    assert select_ref.select_codes(patient, code, 4, 4, None, 2, None, "all")[4].tolist() == [0, 1, 2, 3, 4, 6, 7, 9]
    valid = [1, 1, 0, 1, 1, 1, 1, 1, 1, 1]
    n_pat, _, rank, _, rows = select_ref.select_codes(patient, code, 4, 4, valid, 2, None, "first")
    assert n_pat.tolist() == [2, 1, 0, 2] and rank.tolist() == [0, -1, -1, 1] and rows.tolist() == [3, 6, 7, 9]


def test_library_exports_the_selection():
    from mmgnn import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "mmg_code_select") and hasattr(raw, "mmg_code_select_ws_bytes")
    assert {"mmg_code_select", "mmg_code_select_ws_bytes"} <= set(_lib.SIGNATURES)


def test_c_abi_argument_errors_without_a_gpu():
    from mmgnn import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    nul = ctypes.c_void_p(None)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40
    cnt = ctypes.c_int64(7)
    ref = ctypes.byref(cnt)

    def call(n=10, n_patients=4, n_codes=3, mode=0, code=p, patient=p, outs=(p, p, p, p), out_rows=p, n_out=ref, ws=p,
             ws_bytes=big):
        return lib.mmg_code_select(code, patient, nul, n, n_patients, n_codes, 1, -1, mode, *outs, out_rows, n_out, ws,
                                   ws_bytes, nul)

    def refused(rc, *words):
        msg = lib.mmg_last_error()
        assert rc == -1 and all(w in msg for w in words), (rc, msg)

    refused(call(n=-1), b"code_select", b" n -1")
    refused(call(n=1 << 31), b" n 2147483648")
    refused(call(n_codes=0), b"n_codes 0")
    refused(call(n_patients=0), b"n_patients 0")
    refused(call(n_codes=1 << 40, n_patients=1 << 30), b"n_codes 1099511627776 * n_patients 1073741824", b"63 bits")
    refused(call(n_codes=1 << 31), b"n_codes 2147483648")
    refused(call(n_patients=1 << 31), b"n_patients 2147483648")
    refused(call(mode=2), b"rows_mode 2")
    refused(call(mode=-1), b"rows_mode -1")
    for i in range(4):
        refused(call(outs=tuple(nul if j == i else p for j in range(4))), b"null output")
    refused(call(out_rows=nul), b"out_rows")
    refused(call(n_out=None), b"n_out")
    refused(call(code=nul), b"null input")
    refused(call(patient=nul), b"null input")
    assert cnt.value == 7                                      # nothing was touched
    need = lib.mmg_code_select_ws_bytes(10, 3)
    assert call(ws_bytes=need - 1) == -3 and b"workspace" in lib.mmg_last_error() and b"code_select" in lib.mmg_last_error()
    assert call(ws=nul) == -3 and call(ws_bytes=0) == -3
    # one sort of (8-byte key, 4-byte row) pairs, double-buffered, over the rows and again over the codes
    assert lib.mmg_code_select_ws_bytes(100_000, 5000) > 100_000 * 24 + 5000 * 24
    assert lib.mmg_code_select_ws_bytes(0, 1) > 0
    assert lib.mmg_code_select_ws_bytes(1000, 1 << 20) > (1 << 20) * 24        # n_codes is not capped at 2048


def test_python_layer_refuses_before_the_device(gold):
    from mmgnn import ops
    from mmgnn._lib import MmgError
    z = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(MmgError):
        preprocess.select_codes(z, z, 4, 5000, min_patient_count=1)           # host tensors: no CPU fallback
    with pytest.raises(ValueError, match="rows"):
        ops.code_select(z, z, 4, 4, 1, rows="last")
    with pytest.raises(ValueError, match="n_codes"):
        ops.code_select(z, z, 4, 0, 1)
    with pytest.raises(ValueError, match="one entry per row"):
        ops.code_select(z, z[:3], 4, 4, 1)
    d, meta = gold
    cohort, dx = select_ref.unpack_frame(d, meta, "cohort"), select_ref.unpack_frame(d, meta, "dx/in")
    with pytest.raises(ValueError, match="top_k"):
        preprocess.process_diagnoses(dx, cohort, top_k=-1)


def test_string_codes_are_formed_over_the_unique_values(gold):
    d, meta = gold
    dx = select_ref.unpack_frame(d, meta, "dx/in")
    calls = []

    def rule(t):
        calls.append(t)
        return t[:3]
    codes, keys = preprocess._string_codes(dx["ICD9_CODE"], rule)
    assert len(calls) < 50 < len(dx) and keys.tolist() == sorted(keys.tolist()) and "" not in keys
    text = dx["ICD9_CODE"].astype(str).str.strip()
    assert [None if c < 0 else keys[c] for c in codes] == [t[:3] if t else None for t in text]
    assert {"nan", "Non"} <= set(keys)                         # a missing code is the text pandas gives it


@pytest.mark.parametrize("kind", ["diagnosis", "medication"])
def test_make_code_events(kind):
    ev = make_code_events(1, seed=3, kind=kind)
    n = ev["patient"].numel()
    assert ev["code"].shape == (n,) and ev["patient"].dtype == ev["code"].dtype == torch.int64
    E = ev["edge_index"].shape[1]
    assert ev["n_patients"] == 1834 and ev["n_vocab"] == (114 if kind == "diagnosis" else 100) and ev["n_codes"] >= 2048
    assert E == (5421 if kind == "diagnosis" else 15933) and n > 1.5 * E
    inside = ev["patient"] < ev["n_patients"]
    assert 0 < int((~inside).sum()) < 0.02 * n
    vocab = inside & (ev["code"] < ev["n_vocab"])
    pair = torch.unique(ev["patient"][vocab] * ev["n_vocab"] + ev["code"][vocab])
    assert torch.equal(pair, torch.sort(ev["edge_index"][0] * ev["n_vocab"] + ev["edge_index"][1]).values)   # the graph's edges
    assert pair.numel() < int(vocab.sum())                     # repeated pairs
    tail = ev["code"][inside & (ev["code"] >= ev["n_vocab"])]
    assert torch.unique(tail).numel() > 1900 and int(tail.max()) < ev["n_codes"]
    per_tail = select_ref.select_codes(ev["patient"].numpy(), ev["code"].numpy(), ev["n_patients"], ev["n_codes"])[0]
    assert per_tail[ev["n_vocab"]:].max() < 5                   # the tail stays below the default minimum
    assert not torch.equal(ev["code"], torch.sort(ev["code"]).values)          # shuffled
    ev2 = make_code_events(1, seed=3, kind=kind)
    assert torch.equal(ev["patient"], ev2["patient"]) and torch.equal(ev["code"], ev2["code"])
    assert not torch.equal(ev["patient"], make_code_events(1, seed=4, kind=kind)["patient"])
    frame, cohort = code_event_frames(ev, kind)
    col = "ICD9_CODE" if kind == "diagnosis" else "DRUG"
    assert list(frame.columns) == ["SUBJECT_ID", "HADM_ID", col] and len(frame) == n
    assert list(cohort.columns) == ["SUBJECT_ID", "HADM_ID"] and len(cohort) == 1834
    with pytest.raises(ValueError):
        make_code_events(1, kind="lab")
