"""Host restatements and fixtures for the device graph build (tests/test_graph_device_*.py).  Nothing here touches the
device path: expectations come from pandas / numpy and from mmgnn.graph_build's host builder."""
import numpy as np
import pandas as pd
import torch

from mmgnn import graph_build as gb
from mmgnn.synth import lab_event_frames, make_lab_events


def _keyed(col):
    return np.array([gb._key(x) for x in col], dtype=object)


def sorted_codes(col):
    """ids -> (codes int64, the keys by code): the key rule first, then SORTED uniques, so that code order is not
    first-seen order.  ("V10" sorts behind "303"; "10006" and 10006.0 get one code.)"""
    keys = _keyed(col)
    if len(keys) == 0:
        return np.empty(0, dtype=np.int64), np.empty(0, dtype=object)
    uniq, inv = np.unique(keys.astype(str), return_inverse=True)
    return inv.astype(np.int64).reshape(-1), uniq.astype(object)


def events_to_codes(cohort_ids, labs, dx, med):
    """The four id columns of the frames as codes.  The patient code space is the union of the cohort and of every
    event's patient, so an id unknown to the cohort has a code too (and no index).
    -> (cohort, (p, lab, value), (p, dx), (p, med), n_codes, keys) as numpy arrays."""
    n = [len(cohort_ids), len(labs[0]), len(dx[0]), len(med[0])]
    every = list(cohort_ids) + list(labs[0]) + list(dx[0]) + list(med[0])
    pcode, pkeys = sorted_codes(every)
    cuts = np.cumsum([0] + n)
    pc = [pcode[cuts[i]:cuts[i + 1]] for i in range(4)]
    lcode, lkeys = sorted_codes(labs[1])
    dcode, dkeys = sorted_codes(dx[1])
    mcode, mkeys = sorted_codes(med[1])
    n_codes = {"patient": len(pkeys), "lab": len(lkeys), "diagnosis": len(dkeys), "medication": len(mkeys)}
    keys = {"patient": pkeys, "lab": lkeys, "diagnosis": dkeys, "medication": mkeys}
    value = np.asarray(labs[2], dtype=np.float64)
    return pc[0], (pc[1], lcode, value), (pc[2], dcode), (pc[3], mcode), n_codes, keys


def to_device(arrs, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs)


def first_seen(code, n_codes, valid=None):
    """pd.factorize over the counted rows -> (index_of_code int32 [n_codes], code_of_index int64)."""
    code = np.asarray(code, dtype=np.int64)
    ok = (code >= 0) & (code < n_codes)
    if valid is not None:
        ok &= np.asarray(valid) != 0
    _, uniq = pd.factorize(code[ok])
    uniq = np.asarray(uniq, dtype=np.int64)
    index = np.full(n_codes, -1, dtype=np.int32)
    index[uniq] = np.arange(len(uniq), dtype=np.int32)
    return index, uniq


def edges(patient, item, value, patient_index, item_index):
    """numpy masking -> (fwd int64 [2, E], attr fp32 [E])."""
    patient, item = np.asarray(patient, dtype=np.int64), np.asarray(item, dtype=np.int64)
    ok = (patient >= 0) & (patient < len(patient_index)) & (item >= 0) & (item < len(item_index))
    pi = np.where(ok, patient_index[np.where(ok, patient, 0)], -1)
    ii = np.where(ok, item_index[np.where(ok, item, 0)], -1)
    keep = (pi >= 0) & (ii >= 0)
    fwd = np.stack([pi[keep], ii[keep]]).astype(np.int64)
    with np.errstate(over="ignore"):                     # past the fp32 range: inf, as the conversion rounds it
        return fwd, np.asarray(value, dtype=np.float64)[keep].astype(np.float32)


def chain_fixture():
    """The events of the chain test: synth.make_lab_events(1) cut down to its first 200 patients (and its patients from
    outside the cohort, renumbered behind them) -- about ten thousand events over the eICU x1 vocabulary of 50 labs.
    -> (event tensors on the CPU, the labs frame, the cohort frame)."""
    ev = make_lab_events(1, seed=0, device="cpu", events_per_pair=1.5)
    n_pat = 200
    keep = (ev["patient"] < n_pat) | (ev["patient"] >= ev["n_patients"])
    cut = {k: (v[keep].contiguous() if k in ("patient", "lab", "value", "time") else v) for k, v in ev.items()}
    cut["patient"] = torch.where(cut["patient"] >= ev["n_patients"], cut["patient"] - ev["n_patients"] + n_pat, cut["patient"])
    cut["n_patients"] = n_pat
    del cut["edge_index"]
    labs, cohort = lab_event_frames(cut)
    return cut, labs, cohort
