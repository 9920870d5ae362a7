"""CPU-side checks of dense imputation (no GPU): the C-ABI entry point mmg_pair_head_dense_fwd is declared, exported and
prototyped and rejects bad arguments on the host; the report assembly of mmgnn.inference reproduces the reference's
predict_for_patient dicts on a hand-built case; impute_lab_matrix refuses to run on a CPU model or in training mode."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import fixtures as fx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                 "use_batch_norm": True, "activation": "relu"}}


def test_dense_entry_point_is_declared_exported_and_prototyped():
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    _lib.load()
    assert "mmg_pair_head_dense_fwd(" in open(os.path.join(REPO, "include", "mmgnn.h")).read()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mmg_pair_head_dense_fwd")
    res, args = _lib.SIGNATURES["mmg_pair_head_dense_fwd"]
    assert res is ctypes.c_int and len(args) == 10


def test_dense_argument_errors_are_reported_without_a_gpu():
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(256)                     # never dereferenced: every call below fails on the host
    head = _lib.HeadT(fake, fake, fake, fake, fake, fake)
    rows = out_rows = out = fake

    def call(h=head, r=rows, o_r=out_rows, n=4, n_pat=10, n_labs=5, o=out, n_out=4, ld=5):
        return lib.mmg_pair_head_dense_fwd(ctypes.byref(h) if h is not None else None, r, o_r, n, n_pat, n_labs, o, n_out,
                                           ld, None)

    assert call(n_labs=0) == -1 and b"lab rows" in lib.mmg_last_error()
    assert call(n_labs=-3) == -1
    assert call(ld=4) == -1 and b"ld_out" in lib.mmg_last_error()
    assert call(n=-1) == -1 and b"n_rows" in lib.mmg_last_error()
    assert call(n_pat=0) == -1 and b"patient rows" in lib.mmg_last_error()
    assert call(n_pat=1 << 24) == -1
    assert call(n_out=-1) == -1
    assert call(r=None) == -1 and b"null buffer" in lib.mmg_last_error()
    assert call(o_r=None) == -1 and b"null buffer" in lib.mmg_last_error()
    assert call(o=None) == -1 and b"null buffer" in lib.mmg_last_error()
    assert call(h=None) == -1 and b"null pointer" in lib.mmg_last_error()
    assert call(h=_lib.HeadT(fake, None, fake, fake, fake, fake)) == -1 and b"null pointer" in lib.mmg_last_error()
    assert call(n=0) == 0                           # an empty request enqueues nothing


def test_dense_op_validates_shapes_before_the_device():
    import mmgnn  # noqa: F401
    from mmgnn import ops
    A, B = torch.zeros(6, 64), torch.zeros(5, 64)
    head = ops.Head(A, B, torch.zeros(32, 64), torch.zeros(32), torch.zeros(32), torch.zeros(1))
    r = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="out_rows"):
        ops.pair_head_dense_fwd(head, r, r[:2], torch.zeros(3, 5))
    with pytest.raises(ValueError, match="out must be"):
        ops.pair_head_dense_fwd(head, r, r, torch.zeros(3, 4))
    with pytest.raises(ValueError, match="A and B"):
        ops.pair_head_dense_fwd(ops.Head(torch.zeros(6, 32), B, head.W2, head.b2, head.W3, head.b3), r, r,
                                torch.zeros(3, 5))
    with pytest.raises(Exception, match="HIP device"):
        ops.pair_head_dense_fwd(head, r, r, torch.zeros(3, 5))


def _reference_report(pred_has, pred_missing, lab_indices, values, test_of_edge, lab_stats, lab_indexer):
    """The reference's loop (inference.py:107-178) restated over given predictions: pred_has[i] for the patient's i-th
    edge, pred_missing[name] for a never-measured lab."""
    lab_idx_to_name = {v: k for k, v in lab_indexer.items()}
    measured, masked = {}, {}
    for lab_idx, pred, actual, test in zip(lab_indices, pred_has, values, test_of_edge):
        name = lab_idx_to_name[lab_idx]
        st = lab_stats[lab_stats['ITEMID'] == name].iloc[0]
        a, p = actual * st['std'] + st['mean'], pred * st['std'] + st['mean']
        if test:
            masked[name] = {'predicted': float(p), 'actual': float(a), 'error': float(abs(p - a)),
                            'normalized_predicted': float(pred), 'normalized_actual': float(actual)}
        else:
            measured[name] = {'value': float(a), 'normalized': float(actual)}
    missing = {}
    for name, pred in pred_missing.items():
        st = lab_stats[lab_stats['ITEMID'] == name].iloc[0]
        missing[name] = {'predicted': float(pred * st['std'] + st['mean']), 'normalized_predicted': float(pred),
                         'note': 'Lab was never measured for this patient'}
    return {'measured_labs': measured, 'masked_labs': masked, 'truly_missing_labs': missing}


def test_report_assembly_reproduces_a_hand_built_case():
    import mmgnn  # noqa: F401
    from mmgnn.inference import lab_report
    lab_indexer = {"glucose": 0, "sodium": 1, "potassium": 2, "creatinine": 3, "lactate": 4}
    lab_stats = pd.DataFrame({"ITEMID": ["sodium", "glucose", "potassium", "creatinine", "lactate", "glucose"],
                              "mean": [140.0, 110.0, 4.1, 1.0, 1.8, -1.0],      # (a second glucose row: the first wins)
                              "std": [3.5, 30.0, 0.5, 0.4, 0.9, -1.0]})
    pred_row = np.array([0.25, -1.5, 0.75, 2.0, -0.125], dtype=np.float32)
    labs = np.array([2, 0, 1], dtype=np.int64)               # edge order: potassium, glucose, sodium
    vals = np.array([0.5, -0.25, 1.0], dtype=np.float32)
    test = np.array([False, True, False])
    rep = lab_report(pred_row, labs, vals, test, lab_stats, lab_indexer)
    assert set(rep) == {"measured_labs", "masked_labs", "truly_missing_labs"}
    assert set(rep["measured_labs"]) == {"potassium", "sodium"}
    assert set(rep["masked_labs"]) == {"glucose"}
    assert set(rep["truly_missing_labs"]) == {"creatinine", "lactate"}
    assert set(rep["measured_labs"]["sodium"]) == {"value", "normalized"}
    assert set(rep["masked_labs"]["glucose"]) == {"predicted", "actual", "error", "normalized_predicted",
                                                  "normalized_actual"}
    assert set(rep["truly_missing_labs"]["lactate"]) == {"predicted", "normalized_predicted", "note"}
    # hand-computed: z * std + mean with the lab's own (first) row of lab_stats
    assert rep["measured_labs"]["sodium"] == {"value": 143.5, "normalized": 1.0}
    assert rep["measured_labs"]["potassium"]["value"] == pytest.approx(4.35, rel=1e-6)
    g = rep["masked_labs"]["glucose"]
    assert g["predicted"] == 110.0 + 0.25 * 30.0 and g["actual"] == 110.0 - 0.25 * 30.0
    assert g["error"] == 15.0 and g["normalized_predicted"] == 0.25 and g["normalized_actual"] == -0.25
    assert rep["truly_missing_labs"]["creatinine"]["predicted"] == pytest.approx(1.8, rel=1e-6)
    assert rep["truly_missing_labs"]["lactate"]["normalized_predicted"] == -0.125
    assert rep["truly_missing_labs"]["lactate"]["note"] == "Lab was never measured for this patient"
    # ... and the reference's own loop over the same predictions gives the same dict, value for value
    ref = _reference_report(pred_row[labs], {"creatinine": pred_row[3], "lactate": pred_row[4]}, labs, vals, test,
                            lab_stats, lab_indexer)
    assert rep == ref


def test_report_of_a_patient_without_labs_and_of_one_with_all():
    import mmgnn  # noqa: F401
    from mmgnn.inference import lab_report
    lab_indexer = {"a": 0, "b": 1}
    lab_stats = pd.DataFrame({"ITEMID": ["a", "b"], "mean": [0.0, 10.0], "std": [1.0, 2.0]})
    pred = np.array([0.5, -0.5], dtype=np.float32)
    none = lab_report(pred, np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, bool), lab_stats, lab_indexer)
    assert none["measured_labs"] == {} and none["masked_labs"] == {}
    assert {k: v["predicted"] for k, v in none["truly_missing_labs"].items()} == {"a": 0.5, "b": 9.0}
    full = lab_report(pred, np.array([1, 0]), np.array([1.0, 2.0], np.float32), np.array([True, True]), lab_stats,
                      lab_indexer)
    assert full["truly_missing_labs"] == {} and set(full["masked_labs"]) == {"a", "b"}


def test_impute_on_a_cpu_model_fails_loudly():
    import mmgnn  # noqa: F401
    from mmgnn.model import build_model
    g = fx.graph_from_frames(fx.det_frames(60, 9, 11, 8))
    model = build_model(CFG, (g.node_types, g.edge_types), None)
    model._init_embeddings(g)
    with pytest.raises(RuntimeError, match="inference-only"):
        model.impute_lab_matrix(g)                  # training mode (the default of a fresh module)
    model.eval()
    with pytest.raises(Exception, match="HIP device|no CPU fallback"):
        model.impute_lab_matrix(g)
    from mmgnn import inference
    with pytest.raises(Exception, match="HIP device|no CPU fallback"):
        inference.impute_missing(model, g)


def test_impute_on_a_sharded_model_is_refused():
    import mmgnn  # noqa: F401
    from mmgnn import dist as mdist
    from mmgnn.model import build_model
    g = fx.graph_from_frames(fx.det_frames(60, 9, 11, 8))
    model = build_model(CFG, (g.node_types, g.edge_types), None)
    model._init_embeddings(g)
    model.eval()
    mdist.shard_model(model, object())              # (the collectives are never reached)
    with pytest.raises(NotImplementedError, match="sharded"):
        model.impute_lab_matrix(g)


class _MatrixModel:
    """Stands in for HeteroRGCN in the host flow of mmgnn.inference: impute_lab_matrix hands back rows of a fixed matrix."""

    def __init__(self, table):
        self.table, self.calls = table, []

    def impute_lab_matrix(self, data, patient_indices=None):
        self.calls.append(None if patient_indices is None else patient_indices.tolist())
        return self.table if patient_indices is None else self.table[patient_indices]


def test_predict_for_patients_groups_each_patients_edges_on_the_host():
    """The host side of predict_for_patient(s) against the reference's per-patient edge lookup
    (torch.where(edge_index[0] == p), inference.py:76-90), over a fixed prediction matrix: one impute call per request."""
    import mmgnn  # noqa: F401
    from mmgnn import inference
    from mmgnn.train import EdgeMasker
    g = fx.graph_from_frames(fx.det_frames(120, 8, 9, 7))
    P, L = int(g["patient"].num_nodes), int(g["lab"].num_nodes)
    table = torch.randn(P, L, generator=torch.Generator().manual_seed(3))
    model = _MatrixModel(table)
    masker = EdgeMasker(g)
    patient_indexer = {str(500 + i): i for i in range(P)}
    lab_indexer = {f"item{j}": j for j in range(L)}
    lab_stats = pd.DataFrame({"ITEMID": list(lab_indexer), "mean": np.linspace(1, 9, L), "std": np.linspace(0.5, 2, L)})
    ei, ea = g["patient", "has_lab", "lab"].edge_index, g["patient", "has_lab", "lab"].edge_attr.squeeze()
    deg = torch.bincount(ei[0], minlength=P)
    picks = [int(torch.nonzero(deg == 0)[0]), int(torch.argmax(deg)), 7, 7, 0]
    reps = inference.predict_for_patients([500 + p for p in picks], g, model, "cpu", None, lab_stats, masker,
                                          patient_indexer, lab_indexer)
    assert model.calls == [picks]
    for p, rep in zip(picks, reps):
        sel = ei[0] == p
        pos = torch.where(sel)[0].numpy()
        labs = ei[1][sel].numpy()
        want = _reference_report(table[p].numpy()[labs], {f"item{j}": table[p].numpy()[j] for j in range(L)
                                                          if j not in set(labs.tolist())},
                                 labs, ea[sel].numpy(), masker.test_mask.numpy()[pos], lab_stats, lab_indexer)
        assert rep == want, p
    one = inference.predict_for_patient(500 + picks[1], g, model, "cpu", None, lab_stats, masker, patient_indexer,
                                        lab_indexer)
    assert one == reps[1] and model.calls[-1] == [picks[1]]
    pred, obs = inference.impute_missing(model, g, torch.tensor([3, 3, 0]))
    want = torch.zeros(P, L, dtype=torch.bool)
    want[ei[0], ei[1]] = True
    assert torch.equal(pred, table[[3, 3, 0]]) and torch.equal(obs, want[[3, 3, 0]])
