"""Host side of the device graph build (csrc/graph.hip, mmgnn.graph_build.build_graph_from_events), no GPU: every
argument of mmg_first_seen_index / mmg_edge_build is refused before anything is enqueued (the fake buffers are never
touched), a short workspace is MMG_E_WS, and the Python entry refuses host tensors and an unreadable config."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import _lib, graph_build as gb, ops
from graph_ref import chain_fixture

E_ARG, E_WS = -1, -3
CFG = {"graph": {"edge_types": {k: {"enabled": True, "bidirectional": True}
                                for k in ("patient_lab", "patient_diagnosis", "patient_medication")}}}
P = ctypes.c_void_p(256)


def _first_seen(lib, n=10, n_codes=4, code=P, index=P, inverse=P, count="own", ws=P, ws_bytes=None):
    cnt = ctypes.c_int64(7)
    if ws_bytes is None:
        ws_bytes = lib.mmg_first_seen_index_ws_bytes(n, n_codes)
    rc = lib.mmg_first_seen_index(code, None, n, n_codes, index, inverse, ctypes.byref(cnt) if count == "own" else None, ws,
                                  ws_bytes, None)
    return rc, lib.mmg_last_error()


def _edge_build(lib, n=10, npc=5, nic=4, ld=None, patient=P, item=P, value=P, pidx=P, iidx=P, fwd=P, rev=P, attr=P,
                count="own", ws=P, ws_bytes=None):
    cnt = ctypes.c_int64(7)
    if ws_bytes is None:
        ws_bytes = lib.mmg_edge_build_ws_bytes(n)
    rc = lib.mmg_edge_build(patient, item, value, n, pidx, npc, iidx, nic, fwd, rev, n if ld is None else ld, attr,
                            ctypes.byref(cnt) if count == "own" else None, ws, ws_bytes, None)
    return rc, lib.mmg_last_error()


def test_first_seen_index_refuses_bad_arguments():
    lib = _lib.load()
    for kw in (dict(n=-1), dict(n=2 ** 31 - 1), dict(n=2 ** 31), dict(n=2 ** 40), dict(n_codes=0), dict(n_codes=-3),
               dict(n_codes=2 ** 31), dict(code=None), dict(index=None), dict(inverse=None), dict(count=None)):
        rc, msg = _first_seen(lib, **kw)
        assert rc == E_ARG and b"first_seen_index" in msg, (kw, rc, msg)


def test_edge_build_refuses_bad_arguments():
    lib = _lib.load()
    for kw in (dict(n=-1), dict(n=2 ** 31 - 1), dict(n=2 ** 31), dict(npc=0), dict(nic=0), dict(npc=2 ** 31),
               dict(nic=2 ** 31), dict(ld=9), dict(ld=0), dict(patient=None), dict(item=None), dict(pidx=None),
               dict(iidx=None), dict(fwd=None), dict(count=None), dict(value=None)):          # attr without value
        rc, msg = _edge_build(lib, **kw)
        assert rc == E_ARG and b"edge_build" in msg, (kw, rc, msg)


def test_short_or_missing_workspace_is_refused():
    lib = _lib.load()
    for call, need in ((_first_seen, lib.mmg_first_seen_index_ws_bytes(10, 4)), (_edge_build, lib.mmg_edge_build_ws_bytes(10))):
        assert need > 0
        for kw in (dict(ws_bytes=need - 1), dict(ws=None, ws_bytes=need)):
            rc, msg = call(lib, **kw)
            assert rc == E_WS and b"workspace" in msg, (call.__name__, kw, rc, msg)
    # a bad argument wins over the workspace: nothing is sized from it
    assert _first_seen(lib, n=-1, ws_bytes=0)[0] == E_ARG and _edge_build(lib, ld=3, ws_bytes=0)[0] == E_ARG


def test_ws_bytes_is_monotone_in_n():
    lib = _lib.load()
    ns = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 17, 2048 * 2048 + 5, 2 ** 31 - 2]
    for n_codes in (1, 50, 2_000_003):
        sizes = [lib.mmg_first_seen_index_ws_bytes(n, n_codes) for n in ns]
        assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > 4 * ns[-1]
        assert lib.mmg_first_seen_index_ws_bytes(1000, n_codes) >= 4 * n_codes
    sizes = [lib.mmg_edge_build_ws_bytes(n) for n in ns]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > 4 * ns[-1]
    assert lib.mmg_edge_build_ws_bytes(-5) == lib.mmg_edge_build_ws_bytes(0)


def test_python_entries_refuse_host_tensors_and_unreadable_config():
    z = torch.zeros(4, dtype=torch.int64)
    v = torch.zeros(4, dtype=torch.float64)
    n_codes = {"patient": 4, "lab": 4, "diagnosis": 4, "medication": 4}
    with pytest.raises(ValueError, match="HIP device"):
        gb.build_graph_from_events(z, (z, z, v), (z, z), (z, z), n_codes, CFG)
    with pytest.raises(ValueError, match="HIP device"):
        gb.build_graph_from_events(z.numpy(), (z, z, v), (z, z), (z, z), n_codes, CFG)
    with pytest.raises(ValueError, match="HIP device"):
        gb.index_first_seen(z, 4)
    for bad in ({}, {"graph": {}}, {"graph": {"edge_types": {"patient_lab": {"enabled": True, "bidirectional": True}}}},
                {"graph": {"edge_types": dict(CFG["graph"]["edge_types"], patient_medication={"enabled": True})}},
                {"graph": {"edge_types": None}}):
        with pytest.raises(ValueError, match="cannot read config"):
            gb.build_graph_from_events(z, (z, z, v), (z, z), (z, z), n_codes, bad)
    with pytest.raises(ValueError, match="cannot read config"):
        gb.build_graph_from_events(z, (z, z, v), (z, z), (z, z), {"patient": 4}, CFG)
    with pytest.raises(Exception, match="HIP device"):
        ops.first_seen_index(z, 4)
    with pytest.raises(Exception, match="HIP device"):
        ops.edge_build(z, z, z.int(), z.int())


def test_chain_fixture_keeps_the_frame_path_within_one_percent():
    """The chain test compares preprocess_lab_events -> build_graph_from_events with aggregate_lab_values ->
    normalize_lab_values -> build_heterogeneous_graph, cell by cell.  Both preprocessing entries drop a (patient, lab)
    pair without a finite in-cohort value; a cell the two could treat differently is one of a lab with fewer than two
    such pairs (no z-score spread).  Counted here from the events alone, without a GPU: the fixture has none of them
    (the allowance is 1 % of the pairs), every lab occurs, and it is some ten thousand rows."""
    cut, labs, cohort = chain_fixture()
    assert 2000 <= len(labs) <= 20000 and cut["n_labs"] == 50 and len(cohort) == cut["n_patients"] == 200
    inc = labs[labs["SUBJECT_ID"].isin(cohort["SUBJECT_ID"])]
    assert len(inc) < len(labs)                                  # events of patients outside the cohort are in
    pairs = inc.groupby(["SUBJECT_ID", "ITEMID"])["VALUENUM"].agg(lambda s: s.notna().any())
    per_lab = pairs.groupby(level="ITEMID").sum()
    fragile = int(pairs[pairs.index.get_level_values("ITEMID").isin(per_lab[per_lab < 2].index)].sum())
    print(f"chain fixture: {len(labs)} events, {len(pairs)} pairs, {int((~pairs).sum())} pairs without a value, {fragile} "
          f"cells in labs with fewer than two values")
    assert len(pairs) > 1000 and fragile <= 0.01 * len(pairs)
    assert len(pd.unique(inc["ITEMID"])) == 50 and np.isfinite(inc["VALUENUM"]).mean() > 0.98
