"""Dense lab imputation on the device (HeteroRGCN.impute_lab_matrix, mmg_pair_head_dense_fwd, mmgnn.inference):
  * bitwise equal to predict_lab_values over the same (patient, lab) pairs -- same head tables, same per-cell arithmetic --
    at 64 / 128 / 256-d, for the model variants, a vocabulary beyond the LDS table (global-B path) and at x100;
  * within 1e-4 per value of the reference's golden test predictions and of the CPU oracle;
  * request handling: subsets, repeats, empty, out of range, wrong device, training mode, BatchNorm buffers;
  * predict_for_patient / predict_for_patients against the reference's two-forward computation.
"""
import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_io import load, rel_close, rel_err, t
from oracle import fixtures as fx
from oracle import model as om
from oracle import train as ot

CFG = {"model": {"architecture": "RGCN", "hidden_dim": 128, "num_layers": 2, "dropout": 0.0,
                 "use_batch_norm": True, "activation": "relu"}}
SMALL, EICU = (300, 12, 15, 10), (1834, 50, 114, 100)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def make(dev, n, hidden, **model_kw):
    import mmgnn  # noqa: F401
    from mmgnn.model import build_model
    g = fx.graph_from_frames(fx.det_frames(*n))
    gv = om.GraphView(g)
    cfg = {"model": dict(CFG["model"], hidden_dim=hidden, **model_kw)}
    sd = fx.det_state(gv.num_nodes, hidden, num_layers=cfg["model"]["num_layers"])
    if not cfg["model"]["use_batch_norm"]:
        sd = {k: v for k, v in sd.items() if not k.startswith("batch_norms.")}
    model = build_model(cfg, (g.node_types, g.edge_types), None).to(dev)
    gd = g.clone().to(dev)
    model._init_embeddings(gd)
    model.load_state_dict(sd, strict=True)
    model.eval()
    ei, ea = g["patient", "has_lab", "lab"].edge_index, g["patient", "has_lab", "lab"].edge_attr
    return model, g, gd, gv, sd, ei, ea


def all_pairs(P, L, dev):
    return torch.arange(P, device=dev).repeat_interleave(L), torch.arange(L, device=dev).repeat(P)


def assert_bitwise_vs_pairs(model, gd, dev):
    P, L = int(gd["patient"].num_nodes), int(gd["lab"].num_nodes)
    with torch.no_grad():
        dense = model.impute_lab_matrix(gd)
        pi, li = all_pairs(P, L, dev)
        ref = model.predict_lab_values(gd, pi, li).view(P, L)
    assert dense.shape == (P, L) and dense.dtype == torch.float32
    assert torch.isfinite(dense).all()
    diff = int((dense != ref).sum())
    assert torch.equal(dense, ref), f"{diff} of {P * L} cells differ from the pair path"
    deg = torch.bincount(gd["patient", "has_lab", "lab"].edge_index[0], minlength=P)
    assert int((deg < 6).sum()) > 0 and int((deg >= 6).sum()) > 0          # both heads are exercised
    return dense


@pytest.mark.parametrize("n,hidden", [(SMALL, 64), (EICU, 128), (EICU, 256)], ids=["small-64d", "eicu-128d", "eicu-256d"])
def test_dense_matrix_is_bitwise_the_pair_path(dev, n, hidden):
    model, g, gd, *_ = make(dev, n, hidden)
    assert_bitwise_vs_pairs(model, gd, dev)


@pytest.mark.parametrize("tag,n,hidden", [("small", SMALL, 64), ("eicu", EICU, 128)])
def test_dense_matrix_matches_reference_golden(dev, tag, n, hidden):
    gold, meta = load(f"model_{tag}.npz")
    model, g, gd, gv, sd, ei, ea = make(dev, n, hidden)
    tr, va, te = ot.edge_splits(ei.shape[1], 0.7, 0.15, 0.15, 42)
    with torch.no_grad():
        dense = model.impute_lab_matrix(gd).cpu()
    got = dense[ei[0][te], ei[1][te]]
    ok, worst = rel_close(got, t(gold["eval/pred_test"]))
    assert ok, f"element-wise relative error {worst:.2f} x the 1e-4 bar"


def test_dense_matrix_matches_oracle(dev):
    model, g, gd, gv, sd, ei, ea = make(dev, SMALL, 64)
    P, L = gv.num_nodes["patient"], gv.num_nodes["lab"]
    with torch.no_grad():
        dense = model.impute_lab_matrix(gd).cpu()
    pi, li = all_pairs(P, L, "cpu")
    ref, _ = om.predict_lab_values(sd, gv, pi, li)
    assert rel_err(dense.reshape(-1), ref) <= 1e-4


@pytest.mark.parametrize("kw", [dict(num_layers=1), dict(num_layers=3), dict(activation="elu"),
                                dict(use_batch_norm=False)], ids=["layers1", "layers3", "elu", "no-bn"])
def test_model_variants_are_bitwise_the_pair_path(dev, kw):
    model, g, gd, *_ = make(dev, (500, 20, 25, 18), 128, **kw)
    assert_bitwise_vs_pairs(model, gd, dev)


def test_vocabulary_beyond_the_lds_table_is_bitwise_the_pair_path(dev):
    """300 labs > 256: the lab-side table B is read from global memory instead of LDS."""
    model, g, gd, *_ = make(dev, (300, 300, 15, 10), 64)
    assert_bitwise_vs_pairs(model, gd, dev)


def test_subsets_errors_and_buffers(dev):
    import mmgnn  # noqa: F401
    from mmgnn._lib import MmgError
    model, g, gd, gv, sd, ei, ea = make(dev, SMALL, 64)
    P, L = gv.num_nodes["patient"], gv.num_nodes["lab"]
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    with torch.no_grad():
        full = model.impute_lab_matrix(gd)
        rows = torch.tensor([17, 3, P - 1, 17, 0, 250, 3, 3], device=dev)
        sub = model.impute_lab_matrix(gd, rows)
        assert torch.equal(sub, full[rows])
        assert model.impute_lab_matrix(gd, rows.to(torch.int32)).equal(full[rows])
        empty = model.impute_lab_matrix(gd, torch.empty(0, dtype=torch.long, device=dev))
        assert empty.shape == (0, L)
        for bad in ([P], [-1], [0, P + 5]):
            with pytest.raises(IndexError):
                model.impute_lab_matrix(gd, torch.tensor(bad, device=dev))
        with pytest.raises(MmgError):
            model.impute_lab_matrix(gd, torch.tensor([1, 2]))            # host tensor for a device model
    for k, v in model.state_dict().items():
        if k in before:
            assert torch.equal(v, before[k]), k                            # eval: BatchNorm buffers untouched
    model.train()
    with pytest.raises(RuntimeError):
        model.impute_lab_matrix(gd)
    for k, v in model.state_dict().items():
        if k in before:
            assert torch.equal(v, before[k]), k


def test_lazy_embeddings_are_created_on_first_use(dev):
    import mmgnn  # noqa: F401
    from mmgnn.model import build_model
    g = fx.graph_from_frames(fx.det_frames(120, 8, 9, 7)).to(dev)
    model = build_model({"model": dict(CFG["model"], hidden_dim=64)}, (g.node_types, g.edge_types), None).to(dev)
    model.eval()
    assert len(model.embeddings) == 0
    out = model.impute_lab_matrix(g)
    assert len(model.embeddings) == 4 and out.shape == (120, 8) and torch.isfinite(out).all()


def test_full_size_x100(dev):
    """The eICU shape x100 at 128-d: 183,400 x 50 cells -- finite, 1 M random cells bitwise the pair path, and every row
    served by the head its degree selects (shifting one head's output bias moves exactly that head's rows)."""
    import mmgnn  # noqa: F401
    from mmgnn.model import build_model
    from mmgnn.synth import make_graph
    g = make_graph(100, seed=0, device=dev)
    torch.manual_seed(42)
    model = build_model({"model": dict(CFG["model"], hidden_dim=128)}, (g.node_types, g.edge_types), None).to(dev)
    model._init_embeddings(g)
    model.eval()
    P, L = int(g["patient"].num_nodes), int(g["lab"].num_nodes)
    with torch.no_grad():
        dense = model.impute_lab_matrix(g)
        assert dense.shape == (P, L) and bool(torch.isfinite(dense).all())
        gen = torch.Generator(device=dev).manual_seed(7)
        k = torch.randint(0, P * L, (1 << 20,), device=dev, generator=gen)
        pred = model.predict_lab_values(g, k // L, k % L)
        assert torch.equal(dense.view(-1)[k], pred)
        low = torch.bincount(g["patient", "has_lab", "lab"].edge_index[0], minlength=P) < model.degree_threshold
        assert 0 < int(low.sum()) < P
        for which, moved in (("tabular_mlp", low), ("edge_predictor", ~low)):
            b3 = getattr(model, which).mlp[6].bias
            b3 += 1.0
            shifted = model.impute_lab_matrix(g)
            b3 -= 1.0
            assert torch.equal(shifted[~moved], dense[~moved]), which
            assert bool((shifted[moved] != dense[moved]).all()), which


def _indexers_and_stats(P, L):
    patient_indexer = {str(10_000 + 7 * i): i for i in range(P)}
    lab_indexer = {f"lab_{(j * 37) % 1000:03d}": j for j in range(L)}
    rng = np.random.default_rng(3)
    lab_stats = pd.DataFrame({"ITEMID": list(lab_indexer), "mean": rng.normal(50, 20, L), "std": rng.uniform(0.5, 9, L)})
    return patient_indexer, lab_indexer, lab_stats


def _two_forward_report(model, gd, dev, p, lab_stats, masker, lab_indexer):
    """The reference's predict_for_patient (inference.py:72-178): predict_lab_values over the labs the patient has, then
    over the ones it never had."""
    ei, ea = gd["patient", "has_lab", "lab"].edge_index, gd["patient", "has_lab", "lab"].edge_attr.squeeze()
    sel = ei[0] == p
    labs, vals = ei[1][sel].cpu().numpy(), ea[sel].cpu().numpy()
    pos = torch.where(sel)[0].cpu().numpy()
    test = masker.test_mask.cpu().numpy()[pos]
    idx_to_name = {v: k for k, v in lab_indexer.items()}
    with torch.no_grad():
        pred = model.predict_lab_values(gd, torch.full((len(labs),), p, device=dev),
                                        torch.tensor(labs, device=dev)).cpu().numpy()
    measured, masked = {}, {}
    for lab, pr, actual, tst in zip(labs, pred, vals, test):
        name = idx_to_name[lab]
        st = lab_stats[lab_stats['ITEMID'] == name].iloc[0]
        a, q = actual * st['std'] + st['mean'], pr * st['std'] + st['mean']
        if tst:
            masked[name] = {'predicted': float(q), 'actual': float(a), 'error': float(abs(q - a)),
                            'normalized_predicted': float(pr), 'normalized_actual': float(actual)}
        else:
            measured[name] = {'value': float(a), 'normalized': float(actual)}
    missing_names = set(lab_indexer) - set(idx_to_name[i] for i in labs)
    missing = {}
    if missing_names:
        mi = [lab_indexer[nm] for nm in missing_names]
        with torch.no_grad():
            mp = model.predict_lab_values(gd, torch.full((len(mi),), p, device=dev), torch.tensor(mi, device=dev))
        for nm, pr in zip(missing_names, mp.cpu().numpy()):
            st = lab_stats[lab_stats['ITEMID'] == nm].iloc[0]
            missing[nm] = {'predicted': float(pr * st['std'] + st['mean']), 'normalized_predicted': float(pr),
                           'note': 'Lab was never measured for this patient'}
    return {'measured_labs': measured, 'masked_labs': masked, 'truly_missing_labs': missing}


def test_predict_for_patient_matches_the_two_forward_reference(dev):
    import mmgnn  # noqa: F401
    from mmgnn import inference
    from mmgnn.train import EdgeMasker
    model, g, gd, gv, sd, ei, ea = make(dev, EICU, 128)
    P, L = gv.num_nodes["patient"], gv.num_nodes["lab"]
    patient_indexer, lab_indexer, lab_stats = _indexers_and_stats(P, L)
    masker = EdgeMasker(gd)
    deg = torch.bincount(ei[0], minlength=P)
    picks = [int(torch.nonzero(deg == 0)[0]), int(torch.nonzero((deg > 0) & (deg < 6))[0]), int(torch.argmax(deg)), 5]
    for p in picks:
        pid = 10_000 + 7 * p
        got = inference.predict_for_patient(pid, gd, model, dev, None, lab_stats, masker, patient_indexer, lab_indexer)
        assert set(got) == {"measured_labs", "masked_labs", "truly_missing_labs"}
        want = _two_forward_report(model, gd, dev, p, lab_stats, masker, lab_indexer)
        assert got == want, p
        assert len(got["truly_missing_labs"]) == L - len(set(ei[1][ei[0] == p].tolist()))
    ids = [10_000 + 7 * int(p) for p in torch.randperm(P, generator=torch.Generator().manual_seed(5))[:64]]
    many = inference.predict_for_patients(ids, gd, model, dev, None, lab_stats, masker, patient_indexer, lab_indexer)
    assert len(many) == 64
    for pid, rep in zip(ids, many):
        assert rep == inference.predict_for_patient(pid, gd, model, dev, None, lab_stats, masker, patient_indexer,
                                                    lab_indexer)


def test_impute_missing_marks_the_observed_cells(dev):
    import mmgnn  # noqa: F401
    from mmgnn import inference
    model, g, gd, gv, sd, ei, ea = make(dev, SMALL, 64)
    P, L = gv.num_nodes["patient"], gv.num_nodes["lab"]
    pred, obs = inference.impute_missing(model, gd)
    want = torch.zeros(P, L, dtype=torch.bool)
    want[ei[0], ei[1]] = True
    assert torch.equal(obs.cpu(), want)
    with torch.no_grad():
        assert torch.equal(pred, model.impute_lab_matrix(gd))
    rows = torch.tensor([9, 0, 9, P - 1], device=dev)
    p2, o2 = inference.impute_missing(model, gd, rows)
    assert torch.equal(p2, pred[rows]) and torch.equal(o2.cpu(), want[rows.cpu()])
