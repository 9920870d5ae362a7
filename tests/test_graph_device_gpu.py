"""The device graph build (csrc/graph.hip: mmg_first_seen_index, mmg_edge_build; mmgnn.graph_build.build_graph_from_events)
against what never ran on it: the REFERENCE's golden edges (tests/golden/edges_*.npz), the host builder
build_heterogeneous_graph on the same ids, pd.factorize and numpy masking (tests/graph_ref.py).  Everything compared is
integer, or one fp64 -> fp32 rounding: torch.equal / bit patterns throughout.  Frames become codes on the host with SORTED
uniques after the key rule, so code order is not first-seen order."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import _lib, graph_build as gb, ops, preprocess
from mmgnn.data import build_plan
from oracle import fixtures as fx
from golden_io import load, t
import graph_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CFG = {"graph": {"edge_types": {k: {"enabled": True, "bidirectional": True}
                                for k in ("patient_lab", "patient_diagnosis", "patient_medication")}}}
LAB = ("patient", "has_lab", "lab")
ROWS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 17]
BIG = 2048 * 2048 + 5                   # three scan levels


def frames_to_pandas(frames):
    pid, labs, dx, med = frames
    cohort = pd.DataFrame({"SUBJECT_ID": pid})
    labs_df = pd.DataFrame({"SUBJECT_ID": labs[0], "ITEMID": labs[1], "VALUE_NORMALIZED": labs[2]})
    dx_df = pd.DataFrame({"SUBJECT_ID": dx[0], "ICD3_CODE": dx[1]})
    med_df = pd.DataFrame({"SUBJECT_ID": med[0], "DRUG": med[1]})
    labitems = pd.DataFrame({"ITEMID": np.unique(labs[1])})
    return cohort, labs_df, dx_df, med_df, cohort.copy(), labitems


def device_graph(frames, config=CFG, with_keys=True):
    cohort, labs, dx, med, n_codes, keys = graph_ref.events_to_codes(*frames)
    g = gb.build_graph_from_events(graph_ref.to_device([cohort], DEV)[0], graph_ref.to_device(labs, DEV),
                                   graph_ref.to_device(dx, DEV), graph_ref.to_device(med, DEV), n_codes, config,
                                   keys=keys if with_keys else None)
    return g, n_codes, keys


def check_golden(g, gold, meta):
    assert ["|".join(e) for e in g.edge_types] == meta["edge_types"]
    assert g.node_types == ["patient", "lab", "diagnosis", "medication"]
    for et in meta["edge_types"]:
        key = tuple(et.split("|"))
        ei = g[key].edge_index
        assert ei.is_cuda and ei.dtype == torch.int64 and ei.is_contiguous()
        assert torch.equal(ei.cpu(), t(gold["edge_index/" + et])), et
        if "edge_attr/" + et in gold:
            ea = g[key].edge_attr
            assert ea.is_cuda and ea.dtype == torch.float32 and ea.dim() == 2 and ea.shape[1] == 1
            assert torch.equal(ea.cpu().view(torch.int32), t(gold["edge_attr/" + et]).view(torch.int32)), et
    assert [g[n].num_nodes for n in g.node_types] == gold["num_nodes"].tolist()
    assert g["lab", "has_lab_rev", "patient"].edge_attr is g[LAB].edge_attr
    for nt, m in meta["indexers"].items():
        assert g.indexers[nt]["id_to_index"] == m
        assert list(g.indexers[nt]["id_to_index"]) == list(m)           # insertion order too
        assert g.indexers[nt]["index_to_id"] == {i: k for k, i in m.items()}


def same_graph(g, h):
    """Device-built g against host-built h: types, counts and every tensor."""
    assert g.node_types == h.node_types and g.edge_types == h.edge_types
    assert [g[n].num_nodes for n in g.node_types] == [h[n].num_nodes for n in h.node_types]
    for et in h.edge_types:
        a, b = g[et].edge_index, h[et].edge_index
        assert a.dtype == b.dtype == torch.int64 and a.is_contiguous() and tuple(a.shape) == tuple(b.shape), et
        assert torch.equal(a.cpu(), b.cpu()), et
        assert ("edge_attr" in g[et]) == ("edge_attr" in h[et]), et
        if "edge_attr" in h[et]:
            a, b = g[et].edge_attr, h[et].edge_attr
            assert a.dtype == b.dtype == torch.float32 and tuple(a.shape) == tuple(b.shape), et
            assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32)), et


# ---------------------------------------------------------------------------------------------- golden
def test_golden_closed_form_frames(tmp_path):
    gold, meta = load("edges_small.npz")
    frames = fx.det_frames(60, 9, 11, 8)
    g, n_codes, keys = device_graph(frames)
    check_golden(g, gold, meta)
    # the diagnosis codes are first seen in patient order, not in code order: the sorted codes are not the indices
    want = np.array([meta["indexers"]["diagnosis"][k] for k in keys["diagnosis"]])
    assert not np.array_equal(want, np.arange(len(want)))
    # what consumes a graph takes this one as it is
    gb.validate_graph(g)
    st = gb.compute_graph_statistics(g)
    assert st["edge_counts"][LAB] == gold["edge_index/patient|has_lab|lab"].shape[1]
    gb.save_graph(g, tmp_path / "g.pt")
    check_golden_host = gb.load_graph(tmp_path / "g.pt")
    assert torch.equal(check_golden_host[LAB].edge_index, t(gold["edge_index/patient|has_lab|lab"]))
    assert list(check_golden_host.indexers["diagnosis"]["id_to_index"]) == list(meta["indexers"]["diagnosis"])
    plan = build_plan(g, DEV, use_cache=False)
    assert plan.rels[LAB].n_edges == st["edge_counts"][LAB]
    # without keys: the same tensors, no indexers
    h, _, _ = device_graph(frames, with_keys=False)
    assert not hasattr(h, "indexers")
    same_graph(h, g)


def test_golden_quirks_float_string_unknown_repeated_empty():
    gold, meta = load("edges_quirks.npz")
    inp = meta["inputs"]
    frames = (inp["cohort"], tuple(inp["labs"]), tuple(inp["dx"]), ([], []))
    g, n_codes, keys = device_graph(frames)
    assert n_codes == {"patient": 7, "lab": 3, "diagnosis": 4, "medication": 0}      # 10006.0 / "10006": one code
    check_golden(g, gold, meta)
    for et in (("patient", "has_medication", "medication"), ("medication", "has_medication_rev", "patient")):
        assert tuple(g[et].edge_index.shape) == (2, 0) and g[et].edge_index.dtype == torch.int64
    # an empty lab relation has the host builder's shapes as well
    none = (inp["cohort"], ([], [], []), tuple(inp["dx"]), ([], []))
    e, _, _ = device_graph(none)
    assert tuple(e[LAB].edge_index.shape) == (2, 0) and tuple(e[LAB].edge_attr.shape) == (0, 1)
    assert e[LAB].edge_attr.dtype == torch.float32 and e["lab"].num_nodes == 0


# ---------------------------------------------------------------------------------------------- mmg_first_seen_index
def _codes(n, n_codes, seed, stray=True):
    rng = np.random.default_rng(seed)
    code = rng.integers(0, n_codes, n, dtype=np.int64)
    if stray and n:
        where = rng.random(n)
        code = np.where(where < 0.05, -1 - rng.integers(0, 2 ** 40, n), code)
        code = np.where((where >= 0.05) & (where < 0.1), n_codes + rng.integers(0, 2 ** 40, n), code)
        code[rng.integers(0, n)] = np.iinfo(np.int64).max
        code[rng.integers(0, n)] = np.iinfo(np.int64).min
    return code


def _check_first_seen(code, n_codes, valid=None):
    want_index, want_inverse = graph_ref.first_seen(code, n_codes, valid)
    c = torch.from_numpy(code).to(DEV)
    v = torch.from_numpy(valid).to(DEV) if valid is not None else None
    runs = [ops.first_seen_index(c, n_codes, v) for _ in range(2)]
    index, inverse = runs[0]
    assert index.dtype == torch.int32 and inverse.dtype == torch.int64 and tuple(index.shape) == (n_codes,)
    assert inverse.numel() == len(want_inverse)                                          # n_nodes
    assert np.array_equal(index.cpu().numpy(), want_index)
    assert np.array_equal(inverse.cpu().numpy(), want_inverse)
    seen = index[index >= 0].sort().values
    assert torch.equal(seen.cpu(), torch.arange(len(want_inverse), dtype=torch.int32))
    assert torch.equal(runs[1][0], index) and torch.equal(runs[1][1], inverse)           # call to call
    return index, inverse


@pytest.mark.parametrize("n", ROWS)
def test_first_seen_index_against_factorize(n):
    for n_codes in (1, 50, n + 3, 4096, 4097):           # 4096 / 4097: the last LDS table, the first global one
        code = _codes(n, n_codes, seed=n + 7 * n_codes)
        _check_first_seen(code, n_codes)
        rng = np.random.default_rng(n)
        _check_first_seen(code, n_codes, (rng.random(n) < 0.6).astype(np.uint8))
        _check_first_seen(code, n_codes, rng.random(n) < 0.5)                            # a bool mask
        index, inverse = _check_first_seen(code, n_codes, np.zeros(n, dtype=np.uint8))   # every row invalid
        assert inverse.numel() == 0 and bool((index == -1).all())
        if n >= 2 and n_codes >= 2:                       # a code whose only row is the last row
            only = np.where(code == n_codes - 1, 0, code)
            only[-1] = n_codes - 1
            index, inverse = _check_first_seen(only, n_codes)
            assert int(index[n_codes - 1]) == inverse.numel() - 1 and int(inverse[-1]) == n_codes - 1


def test_first_seen_index_mask_moves_an_index():
    code = np.array([3, 1, 3, 2, 1, 0], dtype=np.int64)
    index, inverse = _check_first_seen(code, 5)
    assert index.tolist() == [3, 1, 2, 0, -1] and inverse.tolist() == [3, 1, 2, 0]
    hide = np.array([0, 1, 1, 1, 1, 1], dtype=np.uint8)                  # code 3 is first COUNTED at row 2
    index, inverse = _check_first_seen(code, 5, hide)
    assert index.tolist() == [3, 0, 2, 1, -1] and inverse.tolist() == [1, 3, 2, 0]


@pytest.mark.parametrize("n_codes", [50, 2_000_003])
def test_first_seen_index_at_three_scan_levels(n_codes):
    code = _codes(BIG, n_codes, seed=n_codes)
    index, inverse = _check_first_seen(code, n_codes)
    if n_codes > 50:
        assert int((index == -1).sum()) > n_codes // 10                   # many codes never occur
    else:
        assert inverse.numel() == n_codes


# ---------------------------------------------------------------------------------------------- mmg_edge_build
def _values(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0,
                        1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24), 1.0 + 2.0 ** -24 + 2.0 ** -50,   # ties in fp32
                        3.5e38, -3.5e38, 1e-40, 2.0 ** -150], dtype=np.float64)    # past the fp32 range, subnormal, tie to 0
    if n:
        at = rng.integers(0, n, min(n, 3 * len(special)))
        v[at] = special[np.arange(len(at)) % len(special)]
    return v


def _index_map(n, seed, holes):
    rng = np.random.default_rng(seed)
    m = rng.permutation(n).astype(np.int32)
    if holes:
        m[rng.random(n) < 0.25] = -1
    return m


def _check_edges(patient, item, value, pmap, imap):
    want_fwd, want_attr = graph_ref.edges(patient, item, value, pmap, imap)
    p, i, v, pm, im = graph_ref.to_device((patient, item, value, pmap, imap), DEV)
    fwd, rev, attr = ops.edge_build(p, i, pm, im, v)
    assert fwd.dtype == rev.dtype == torch.int64 and attr.dtype == torch.float32
    assert fwd.is_contiguous() and rev.is_contiguous() and tuple(fwd.shape) == tuple(want_fwd.shape)
    assert np.array_equal(fwd.cpu().numpy(), want_fwd)
    assert torch.equal(rev, fwd.flip(0))
    assert np.array_equal(attr.cpu().numpy().view(np.int32), want_attr.view(np.int32))   # bit for bit, NaN included
    fwd2, rev2, attr2 = ops.edge_build(p, i, pm, im, None, reverse=False)                # rev and attr null
    assert rev2 is None and attr2 is None and torch.equal(fwd2, fwd)
    return fwd, attr


@pytest.mark.parametrize("n", ROWS)
def test_edge_build_against_numpy(n):
    rng = np.random.default_rng(1000 + n)
    npc, nic = 37, 11
    patient = _codes(n, npc, seed=n + 1)                  # ~10 % of the codes out of range; few codes: many duplicates
    item = _codes(n, nic, seed=n + 2)
    value = _values(n, n + 3)
    fwd, attr = _check_edges(patient, item, value, _index_map(npc, n, True), _index_map(nic, n + 1, True))
    if n >= 1024:
        assert 0 < fwd.shape[1] < n
    # no row kept: no patient has an index
    fwd, attr = _check_edges(patient, item, value, np.full(npc, -1, dtype=np.int32), _index_map(nic, n, False))
    assert tuple(fwd.shape) == (2, 0) and tuple(attr.shape) == (0,)
    # every row kept
    patient, item = rng.integers(0, npc, n, dtype=np.int64), rng.integers(0, nic, n, dtype=np.int64)
    fwd, attr = _check_edges(patient, item, value, _index_map(npc, n, False), _index_map(nic, n, False))
    assert fwd.shape[1] == n
    if n >= 1024:
        assert bool(torch.isnan(attr).any()) and bool(torch.isinf(attr).any())
        pairs = fwd[0] * nic + fwd[1]
        assert pairs.unique().numel() < n                  # a repeated pair gives one edge per row


def test_edge_build_with_a_wider_leading_dimension():
    """ld > n through the C entry itself: the two rows of fwd / rev start ld apart, and nothing beyond the kept columns
    is written."""
    n, ld, npc, nic = 1500, 1500 + 77, 37, 11
    patient, item, value = _codes(n, npc, seed=5), _codes(n, nic, seed=6), _values(n, 7)
    pmap, imap = _index_map(npc, 8, True), _index_map(nic, 9, True)
    want_fwd, want_attr = graph_ref.edges(patient, item, value, pmap, imap)
    E = want_fwd.shape[1]
    p, i, v, pm, im = graph_ref.to_device((patient, item, value, pmap, imap), DEV)
    fwd = torch.full((2, ld), -7, dtype=torch.int64, device=DEV)
    rev = torch.full((2, ld), -7, dtype=torch.int64, device=DEV)
    attr = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    cnt = ctypes.c_int64(-1)
    ops._call("mmg_edge_build", p, i, v, n, pm, npc, im, nic, fwd, rev, ld, attr, ctypes.byref(cnt),
              ws=_lib.load().mmg_edge_build_ws_bytes(n))
    assert cnt.value == E and 0 < E < n
    assert np.array_equal(fwd[:, :E].cpu().numpy(), want_fwd) and torch.equal(rev[:, :E], fwd[:, :E].flip(0))
    assert np.array_equal(attr[:E].cpu().numpy().view(np.int32), want_attr.view(np.int32))
    assert bool((fwd[:, E:] == -7).all()) and bool((rev[:, E:] == -7).all()) and bool((attr[E:] == -7.0).all())


# ---------------------------------------------------------------------------------------------- the builder
def test_disabled_and_unidirectional_relations():
    cfg = {"graph": {"edge_types": {"patient_lab": {"enabled": True, "bidirectional": False},
                                    "patient_diagnosis": {"enabled": False, "bidirectional": True},
                                    "patient_medication": {"enabled": True, "bidirectional": True}}}}
    frames = fx.det_frames(40, 6, 5, 4)
    h = gb.build_heterogeneous_graph(*frames_to_pandas(frames), cfg)
    g, _, _ = device_graph(frames, cfg)
    assert g.edge_types == h.edge_types == [("patient", "has_lab", "lab"), ("patient", "has_medication", "medication"),
                                            ("medication", "has_medication_rev", "patient")]
    same_graph(g, h)
    assert g.indexers["diagnosis"]["id_to_index"] == h.indexers["diagnosis"]["id_to_index"]   # indexed though disabled


def test_through_the_model_at_the_x1_shape():
    from mmgnn.model import build_model
    from mmgnn.synth import make_graph
    src = make_graph(1, seed=3, device="cpu", with_reverse=False)
    n_pat = int(src["patient"].num_nodes)
    pid = 10000 + 3 * np.arange(n_pat, dtype=np.int64)
    pid = pid[np.random.default_rng(0).permutation(n_pat)]                 # cohort order is not id order
    lab_e = src[LAB].edge_index.numpy()
    dx_e = src["patient", "has_diagnosis", "diagnosis"].edge_index.numpy()
    med_e = src["patient", "has_medication", "medication"].edge_index.numpy()
    dx_codes = np.array([f"{300 + 3 * j}" if j % 4 else f"V{10 + j}" for j in range(int(src["diagnosis"].num_nodes))], dtype=object)
    med_names = np.array([f"drug_{j:03d}" for j in range(int(src["medication"].num_nodes))], dtype=object)
    frames = (pid, (pid[lab_e[0]], 50800 + 7 * lab_e[1], src[LAB].edge_attr.squeeze(-1).numpy().astype(np.float64)),
              (pid[dx_e[0]], dx_codes[dx_e[1]]), (pid[med_e[0]], med_names[med_e[1]]))
    h = gb.build_heterogeneous_graph(*frames_to_pandas(frames), CFG)
    g, _, _ = device_graph(frames)
    assert g[LAB].edge_index.shape[1] == 61484
    same_graph(g, h)
    for nt in h.node_types:
        assert g.indexers[nt]["id_to_index"] == h.indexers[nt]["id_to_index"]
        assert list(g.indexers[nt]["id_to_index"]) == list(h.indexers[nt]["id_to_index"])
    hd = h.to(DEV)
    pg, ph = build_plan(g, DEV, use_cache=False), build_plan(hd, DEV, use_cache=False)
    assert pg.edge_types == ph.edge_types and pg.num_nodes == ph.num_nodes
    for et in ph.edge_types:
        for f in ("rowptr", "col", "perm"):
            assert torch.equal(getattr(pg.rels[et], f), getattr(ph.rels[et], f)), (et, f)
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"}}
    outs = []
    for graph in (g, hd):
        torch.manual_seed(1)
        model = build_model(cfg, (graph.node_types, graph.edge_types), None).to(DEV)
        model.eval()
        with torch.no_grad():
            outs.append(model(graph))
    assert set(outs[0]) == set(outs[1])
    for k in outs[1]:
        assert torch.isfinite(outs[1][k]).all()
        assert torch.equal(outs[0][k].view(torch.int32), outs[1][k].view(torch.int32)), k


def test_chain_preprocessing_to_graph():
    """Raw lab events -> preprocess_lab_events -> build_graph_from_events, all on the device, against the frame chain
    aggregate_lab_values -> normalize_lab_values -> build_heterogeneous_graph on the same events.  Both preprocessing
    entries run the same aggregation and fit the same table on the same (lab, patient) order, so no cell of this fixture
    is left out of the comparison (tests/test_graph_device_cpu.py counts the cells that could be: none)."""
    ev, labs, cohort = graph_ref.chain_fixture()
    n_pat, n_labs = ev["n_patients"], ev["n_labs"]
    agg = preprocess.aggregate_lab_values(labs, cohort, "last", True, 5.0)
    norm, _ = preprocess.normalize_lab_values(agg, "zscore")
    empty_dx = pd.DataFrame({"SUBJECT_ID": pd.Series([], dtype=np.int64), "ICD3_CODE": pd.Series([], dtype=object)})
    empty_med = pd.DataFrame({"SUBJECT_ID": pd.Series([], dtype=np.int64), "DRUG": pd.Series([], dtype=object)})
    labitems = pd.DataFrame({"ITEMID": np.arange(n_labs)})
    h = gb.build_heterogeneous_graph(cohort, norm, empty_dx, empty_med, cohort, labitems, CFG)

    p, l, v, vn, _ = preprocess.preprocess_lab_events(ev["patient"].to(DEV), ev["lab"].to(DEV), ev["value"].to(DEV),
                                                      ev["time"].to(DEV), n_pat, n_labs, "last", 5.0, "zscore")
    z = torch.zeros(0, dtype=torch.int64, device=DEV)
    g = gb.build_graph_from_events(torch.arange(n_pat, device=DEV), (p, l, vn), (z, z), (z, z),
                                   {"patient": n_pat, "lab": n_labs, "diagnosis": 0, "medication": 0}, CFG,
                                   keys={"patient": np.arange(n_pat), "lab": np.arange(n_labs)})
    left_out = 0                                          # cells excluded from the comparison (allowed: 1 % of the pairs)
    assert left_out <= 0.01 * len(norm)
    same_graph(g, h)
    assert g[LAB].edge_index.shape[1] == len(norm) > 5000
    for nt in ("patient", "lab"):
        assert g.indexers[nt]["id_to_index"] == h.indexers[nt]["id_to_index"]
    ei = g[LAB].edge_index.cpu()
    for e in (ei, h[LAB].edge_index):                     # lab-major, patients ascending inside a lab
        step_lab, step_pat = e[1][1:] - e[1][:-1], e[0][1:] - e[0][:-1]
        assert bool((step_lab >= 0).all()) and bool((step_pat[step_lab == 0] > 0).all())
