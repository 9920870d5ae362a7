"""Leakage audit on the MI355X: exact order statistics (mmg_order_stats) against np.partition, numpy's percentile bit for
bit, the robust metrics (mmg_robust_sums) against the fp64 and fp32 restatements (audit_ref.py), bitwise
reproducibility and hipGraph capture, split membership and holdout masks at x100, Trainer on a PatientHoldoutSplitter,
and run_full_audit's device path against its host path."""
import json
import os

import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import audit, ops
from mmgnn.train import LAB_EDGE, EdgeMasker
from oracle import fixtures as fx
import audit_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audit_small.npz")


def _same_values(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    return bool(np.all(both_nan | (got == want)))


def _dist(kind, n, rng):
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "equal":
        return np.full(n, -2.5, np.float32)
    if kind == "ties":
        return rng.integers(-3, 4, n).astype(np.float32)
    if kind == "negative":
        return -np.abs(rng.standard_normal(n).astype(np.float32)) * 1e3
    if kind == "zeros":
        return np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    if kind == "denormal":
        x = (rng.integers(-50, 50, n) * np.float32(1e-44)).astype(np.float32)
        return x
    if kind == "inf":
        x = rng.standard_normal(n).astype(np.float32)
        x[rng.random(n) < 0.1] = np.inf
        x[rng.random(n) < 0.1] = -np.inf
        return x
    if kind == "nan":
        x = rng.standard_normal(n).astype(np.float32)
        x[rng.random(n) < 0.05] = np.nan
        x[0] = np.nan
        return x
    raise ValueError(kind)


def _ranks(n, rng):
    r = {0, n - 1, n // 2, max(0, n - 2), min(n - 1, 1)}
    r |= {int(v) for v in rng.integers(0, n, 3)}
    return sorted(r)[:8]


KINDS = ["normal", "equal", "ties", "negative", "zeros", "denormal", "inf", "nan"]


@pytest.mark.parametrize("n", [1, 2, 3, 1000, (1 << 20) + 7])
@pytest.mark.parametrize("kind", KINDS)
def test_order_stats_equal_np_partition(n, kind):
    rng = np.random.default_rng(n * 31 + KINDS.index(kind))
    x = _dist(kind, n, rng)
    ranks = _ranks(n, rng)
    vals, nanc = ops.order_stats(torch.from_numpy(x).to(DEV), ranks)
    want = np.partition(x, ranks)[ranks]
    assert _same_values(vals.cpu().numpy(), want), (kind, n, vals.cpu().numpy(), want)
    assert int(nanc.item()) == int(np.isnan(x).sum())
    # |a - b| mode
    y = _dist("normal", n, rng)
    vals, _ = ops.order_stats(torch.from_numpy(x).to(DEV), ranks, b=torch.from_numpy(y).to(DEV))
    key = np.abs(x - y)
    assert _same_values(vals.cpu().numpy(), np.partition(key, ranks)[ranks]), (kind, n)


@pytest.mark.parametrize("kind", ["normal", "ties"])
def test_order_stats_at_2e7(kind):
    n = 20_000_000
    rng = np.random.default_rng(5)
    x = _dist(kind, n, rng)
    ranks = _ranks(n, rng)
    vals, _ = ops.order_stats(torch.from_numpy(x).to(DEV), ranks)
    assert _same_values(vals.cpu().numpy(), np.partition(x, ranks)[ranks])


def _percentiles(x, pct):
    s = audit.robust_sums_device(torch.zeros(x.size, device=DEV), torch.from_numpy(x).to(DEV), pct).cpu().numpy()
    return np.float32(s[12]), np.float32(s[13]), np.float32(s[14])


def test_percentiles_bit_equal_numpy():
    rng = np.random.default_rng(11)
    checked = 0
    sizes = list(range(1, 41)) + [97, 1000, 4096, 65537]
    for n in sizes:
        x = np.abs(rng.standard_normal(n).astype(np.float32)) * 2
        if n > 8:
            x[: n // 4] = x[0]                          # ties
        for pct in [0.0, 5.0, 50.0, 100.0] + [float(v) for v in rng.uniform(0, 100, 30)]:
            lo, hi, q95 = _percentiles(x, pct)
            for got, p in ((lo, pct), (hi, 100 - pct)):
                want = np.float32(np.percentile(x, p))
                assert got.view(np.uint32) == want.view(np.uint32), (n, p, got, want)
                checked += 1
        assert q95.view(np.uint32) == np.float32(np.percentile(x, 95)).view(np.uint32)
    # n - 1 > 2^24: the virtual index (n - 1) * q rounds in fp32
    n = (1 << 24) + 5
    x = np.abs(rng.standard_normal(n).astype(np.float32))
    for pct in [5.0, 33.3, 50.0, 95.0, 99.99]:
        lo, hi, _ = _percentiles(x, pct)
        for got, p in ((lo, pct), (hi, 100 - pct)):
            assert got.view(np.uint32) == np.float32(np.percentile(x, p)).view(np.uint32), (n, p)
            checked += 1
    assert checked >= 3000
    xn = np.array([1.0, np.nan, 3.0], np.float32)
    assert all(np.isnan(v) for v in _percentiles(xn, 5.0))


def _robust_cases():
    d = np.load(GOLDEN)
    cases = {k[len("robust_"):-len("_true")]: (d[k], d[k.replace("_true", "_pred")])
             for k in d.files if k.startswith("robust_") and k.endswith("_true")}
    meta = json.loads(str(d["__meta__"]))["robust"]
    rng = np.random.default_rng(2)
    t = rng.standard_normal(1_000_003).astype(np.float32)
    cases["big"] = (t, (t + 0.3 * rng.standard_normal(t.size) + 0.02 * rng.standard_cauchy(t.size)).astype(np.float32))
    return cases, meta


INT_FIELDS = ("num_outliers_capped", "winsorize_percentile")


def _rel(a, b):
    if np.isnan(b):
        return 0.0 if np.isnan(a) else np.inf
    if np.isinf(b):
        return 0.0 if a == b else np.inf
    return abs(a - b) / max(abs(b), 1e-300)


def test_robust_metrics_match_the_restatements():
    cases, meta = _robust_cases()
    for name, (yt, yp) in cases.items():
        pct = meta[name]["winsorize_percentile"] if name in meta else 5.0
        got = audit.compute_robust_metrics(torch.from_numpy(yt).to(DEV), torch.from_numpy(yp).to(DEV), pct)
        with np.errstate(all="ignore"):
            f64 = audit_ref.robust_metrics_f64(yt, yp, pct)
            f32 = audit_ref.robust_metrics_f32(yt, yp, pct)
        assert set(got) == set(f32)
        for k in got:
            if k in INT_FIELDS:
                assert got[k] == f64[k] == f32[k], (name, k)
                continue
            assert _rel(got[k], f64[k]) <= 1e-12, (name, k, got[k], f64[k])
            if k == "r2":            # 1 - SSres / SStot: compare the ratio, the fp32 sums' own error sits there
                assert _rel(1 - got[k], 1 - f32[k]) <= 2e-6, (name, k, got[k], f32[k])
            else:
                assert _rel(got[k], f32[k]) <= 2e-6, (name, k, got[k], f32[k])
        if name in meta:
            for k in ("max_residual", "p95_residual"):
                assert _rel(got[k], meta[name][k]) == 0.0, (name, k)


def test_robust_sums_reproducible_and_capturable():
    rng = np.random.default_rng(4)
    yt = torch.from_numpy(rng.standard_normal(3_000_001).astype(np.float32)).to(DEV)
    yp = yt + 0.5 * torch.randn(yt.numel(), device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    runs = [audit.robust_sums_device(yt, yp).cpu() for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r.view(torch.int64), runs[0].view(torch.int64))
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        audit.robust_sums_device(yt, yp)                  # warm-up off the default stream, as torch.cuda.graph asks
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(g):
        out = audit.robust_sums_device(yt, yp)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int64), runs[0].view(torch.int64))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int64), runs[0].view(torch.int64))


@pytest.fixture(scope="module")
def x100():
    from mmgnn.synth import make_graph
    g = make_graph(100, seed=0, device=DEV)
    return g


def test_split_membership_at_x100(x100):
    g = x100
    ei = g[LAB_EDGE].edge_index
    em = EdgeMasker(g, 0.7, 0.15, 0.15, 0.2, 42)
    hs = audit.PatientHoldoutSplitter(g, 0.7, 0.15, 0.15, seed=42)
    ei_np = ei.cpu().numpy()
    for m in (em, hs):
        assert m.train_mask.is_cuda
        got = audit.audit_patient_leakage(ei, m.train_mask, m.val_mask, m.test_mask)
        masks = [t.cpu().numpy() for t in (m.train_mask, m.val_mask, m.test_mask)]
        assert got == audit_ref.patient_sets_report(ei_np, *masks)
        host = audit.audit_patient_leakage(ei.cpu(), *(t.cpu() for t in (m.train_mask, m.val_mask, m.test_mask)))
        assert host == got
    rep = audit.audit_masked_value_visibility(g, em)
    assert rep["supervision_leak"] is False
    c = ops.split_membership(ei[0].contiguous(), em.train_mask, em.val_mask | em.train_mask, em.test_mask,
                             int(g["patient"].num_nodes)).cpu().tolist()
    assert c[8] == c[9] == int(em.train_mask.sum())


def test_holdout_masks_at_x100(x100):
    g = x100
    pid = g[LAB_EDGE].edge_index[0]
    hs = audit.PatientHoldoutSplitter(g, 0.7, 0.15, 0.15, seed=42)
    # the vectorised restatement of the reference's split
    uniq = torch.unique(pid.cpu())
    torch.manual_seed(42)
    perm = torch.randperm(len(uniq))
    n_tr, n_va = int(0.7 * len(uniq)), int(0.15 * len(uniq))
    p_np = pid.cpu().numpy()
    parts = (perm[:n_tr], perm[n_tr:n_tr + n_va], perm[n_tr + n_va:])
    for part, mask, pats in zip(parts, (hs.train_mask, hs.val_mask, hs.test_mask),
                                (hs.train_patients, hs.val_patients, hs.test_patients)):
        want = np.isin(p_np, uniq[part].numpy())
        assert np.array_equal(mask.cpu().numpy(), want)
        assert pats == set(uniq[part].tolist())
    assert int((hs.train_mask.int() + hs.val_mask.int() + hs.test_mask.int() != 1).sum()) == 0
    sub = torch.randperm(pid.numel(), generator=torch.Generator().manual_seed(0))[:20000]
    loop = audit_ref.holdout_masks_loop(pid.cpu()[sub], hs.train_patients, hs.val_patients, hs.test_patients)
    for a, b in zip(loop, (hs.train_mask, hs.val_mask, hs.test_mask)):
        assert torch.equal(a, b.cpu()[sub])


def _config(epochs=4):
    return {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                      "use_batch_norm": True, "activation": "relu"},
            "train": {"optimizer": {"type": "adam", "lr": 5e-3, "weight_decay": 1e-5, "momentum": 0.0},
                      "lr_scheduler": {"enabled": True, "type": "step", "step_size": 2, "gamma": 0.5},
                      "loss": "mae", "epochs": epochs, "early_stopping_patience": 20, "train_split": 0.7,
                      "val_split": 0.15, "test_split": 0.15, "mask_fraction": 0.2, "seed": 42, "device": "cuda"},
            "logging": {"save_checkpoints": True, "checkpoint_interval": 2}}


def _model(cfg, g, sd):
    from mmgnn.model import build_model
    model = build_model(cfg, (g.node_types, g.edge_types), None)
    model._init_embeddings(g)
    model.load_state_dict(sd)
    return model


def test_trainer_on_patient_holdout_split(tmp_path):
    from mmgnn.train import Trainer
    from oracle import model as om
    n = (300, 12, 15, 10)
    cfg = _config()
    g0 = fx.graph_from_frames(fx.det_frames(*n))
    sd = fx.det_state(om.GraphView(g0).num_nodes, 64)
    out = []
    for device_step in (False, True):
        g = fx.graph_from_frames(fx.det_frames(*n))
        hs = audit.PatientHoldoutSplitter(g, 0.7, 0.15, 0.15, seed=42,
                                          mask_generator=torch.Generator().manual_seed(11))
        model = _model(cfg, g, sd)
        tr = Trainer(model, g, hs, cfg, DEV, device_step=device_step)
        hist = tr.train(tmp_path / str(device_step))
        out.append((hist, tr, hs))
    (he, te, _), (hg, tg, hs) = out
    assert tg._dstep is not None and te._dstep is None
    for k in ("train_loss", "val_loss"):
        assert len(hg[k]) == len(he[k]) == 4
        for a, b in zip(hg[k], he[k]):
            assert abs(a - b) <= 2e-4 * abs(b), (k, hg[k], he[k])
    assert hg["learning_rates"] == he["learning_rates"]
    ei, _, _, _ = hs.get_masked_data("val")
    val_patients = set(ei[0].cpu().tolist())
    assert val_patients and val_patients <= hs.val_patients and not (val_patients & hs.train_patients)


def test_run_full_audit_device_equals_host(tmp_path):
    n = (300, 12, 15, 10)
    cfg = _config()
    from oracle import model as om
    g = fx.graph_from_frames(fx.det_frames(*n))
    sd = fx.det_state(om.GraphView(g).num_nodes, 64)
    model = _model(cfg, g, sd).to(DEV)
    dev_rep = audit.run_full_audit(model, g, cfg, tmp_path / "dev")
    host_rep = audit.run_full_audit(model, g, cfg, tmp_path / "host", device_reducers=False)
    assert set(dev_rep) == {"leakage_check", "patient_distribution", "split_comparison", "robust_metrics"}
    on_disk = json.load(open(tmp_path / "dev" / "audit_report.json"))
    assert on_disk["patient_distribution"] == dev_rep["patient_distribution"]
    for k in ("leakage_check", "patient_distribution", "split_comparison"):
        assert dev_rep[k] == host_rep[k], k
    for k, v in host_rep["robust_metrics"].items():
        d = dev_rep["robust_metrics"][k]
        if k == "r2":                # 1 - SSres / SStot: the ratio to 1e-6 (the host's fp32 sums carry its error)
            d, v = 1 - d, 1 - v
        assert _rel(d, v) <= 1e-6, (k, dev_rep["robust_metrics"][k], host_rep["robust_metrics"][k])
    assert dev_rep["robust_metrics"]["num_outliers_capped"] == host_rep["robust_metrics"]["num_outliers_capped"]
