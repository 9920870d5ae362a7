"""Leakage audit on the host: the numpy restatement (audit_ref.py) and the host paths of mmgnn.audit against what the
reference's own audit_leakage functions returned (tests/golden/audit_small.npz), numpy's percentile arithmetic, the
C-ABI argument checks and the ops wrappers' refusal of host tensors."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import audit, ops
from mmgnn._lib import MmgError
from mmgnn.train import LAB_EDGE, EdgeMasker
from oracle import fixtures as fx
import audit_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audit_small.npz")
GRAPHS = {"small": (300, 12, 15, 10), "eicu": (1834, 50, 114, 100)}


@pytest.fixture(scope="module")
def gold():
    d = np.load(GOLDEN)
    return d, json.loads(str(d["__meta__"]))


def _close(got, want, rel=1e-6):
    for k, w in want.items():
        g = got[k]
        if isinstance(w, str) or isinstance(w, int) and not isinstance(w, bool):
            assert g == w, (k, g, w)
        elif np.isnan(w):
            assert np.isnan(g), (k, g)
        elif np.isinf(w):
            assert g == w, (k, g, w)
        else:
            assert abs(g - w) <= rel * max(abs(w), 1e-30), (k, g, w)
    assert set(got) == set(want)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_holdout_masks_are_the_reference_masks(gold, name):
    d, meta = gold
    g = fx.graph_from_frames(fx.det_frames(*GRAPHS[name]))
    hs = audit.PatientHoldoutSplitter(g, 0.7, 0.15, 0.15, seed=42)
    E = int(d[f"{name}_edges"])
    for split in ("train", "val", "test"):
        want = np.unpackbits(d[f"{name}_holdout_{split}"])[:E].astype(bool)
        assert np.array_equal(getattr(hs, f"{split}_mask").numpy(), want), split
    m = meta["graphs"][name]
    assert hs.num_patients == m["num_patients"] == len(hs.unique_patients)
    assert (len(hs.train_patients), len(hs.val_patients), len(hs.test_patients)) == (
        m["n_train_patients"], m["n_val_patients"], m["n_test_patients"])
    assert isinstance(hs.train_patients, set) and isinstance(hs, EdgeMasker)
    # the reference's loop over the edges gives the same masks
    loop = audit_ref.holdout_masks_loop(g[LAB_EDGE].edge_index[0][:3000], hs.train_patients, hs.val_patients,
                                        hs.test_patients)
    for a, b in zip(loop, (hs.train_mask, hs.val_mask, hs.test_mask)):
        assert torch.equal(a, b[:3000])


@pytest.mark.parametrize("name", list(GRAPHS))
def test_patient_distribution_reports(gold, name):
    _, meta = gold
    g = fx.graph_from_frames(fx.det_frames(*GRAPHS[name]))
    ei = g[LAB_EDGE].edge_index
    em = EdgeMasker(g, 0.7, 0.15, 0.15, 0.2, 42)
    hs = audit.PatientHoldoutSplitter(g, 0.7, 0.15, 0.15, seed=42)
    for masker, key in ((em, "edge_level"), (hs, "holdout")):
        want = meta["graphs"][name][key]
        got = audit.audit_patient_leakage(ei, masker.train_mask, masker.val_mask, masker.test_mask)
        assert got == want
        assert audit_ref.patient_sets_report(ei.numpy(), masker.train_mask.numpy(), masker.val_mask.numpy(),
                                             masker.test_mask.numpy()) == want
    cmp = audit.compare_split_strategies(g, {"train": {"train_split": 0.7, "val_split": 0.15, "test_split": 0.15,
                                                       "seed": 42, "device": "cpu"}})
    assert set(cmp) == {"edge_level_split", "patient_holdout_split", "recommendation"}
    assert cmp["edge_level_split"] == meta["graphs"][name]["edge_level"]
    hold = dict(meta["graphs"][name]["holdout"], split_type="patient_holdout",
                note="Patient-holdout: NO patient overlap (more conservative)")
    assert cmp["patient_holdout_split"] == hold


def test_masked_value_visibility():
    g = fx.graph_from_frames(fx.det_frames(300, 12, 15, 10))
    em = EdgeMasker(g, 0.7, 0.15, 0.15, 0.2, 42)
    rep = audit.audit_masked_value_visibility(g, em)
    assert rep["supervision_leak"] is False and rep["masked_values_in_node_features"] is False
    assert rep["supervision_leak_details"] == "✓ Train/val/test masks are mutually exclusive"
    em.val_mask = em.val_mask.clone()
    em.val_mask[torch.nonzero(em.train_mask)[0]] = True
    rep = audit.audit_masked_value_visibility(g, em)
    assert rep["supervision_leak"] is True and rep["supervision_leak_details"] == "Train mask overlaps with val/test!"


def test_robust_metrics_host_paths_match_the_reference(gold):
    d, meta = gold
    for name, want in meta["robust"].items():
        yt, yp = d[f"robust_{name}_true"], d[f"robust_{name}_pred"]
        pct = want["winsorize_percentile"]
        with np.errstate(all="ignore"):
            _close(audit.compute_robust_metrics(yt, yp, winsorize_pct=pct), want)
            _close(audit_ref.robust_metrics_f32(yt, yp, pct), want)
            f64 = audit_ref.robust_metrics_f64(yt, yp, pct)
            assert f64["num_outliers_capped"] == want["num_outliers_capped"], name
            for k in ("mae", "rmse", "smape", "mae_winsorized", "rmse_winsorized", "p95_residual", "max_residual"):
                w = want[k]
                assert (np.isnan(w) and np.isnan(f64[k])) or abs(f64[k] - w) <= 2e-6 * abs(w) + 1e-12, (name, k)
            # the device's derivation from the 15 sums gives the same dict
            _close(audit.robust_metrics_from_sums(audit_ref.robust_sums_f64(yt, yp, pct), pct), f64, rel=1e-12)


def test_percentile_plan_is_numpy_bit_for_bit():
    rng = np.random.default_rng(3)
    for n in list(range(1, 70)) + [1000, 4097, 65536]:
        x = np.sort((rng.standard_normal(n) * 3).astype(np.float32))
        if n > 4:
            x[1:4] = x[1]
        for pct in [0.0, 5.0, 95.0, 100.0, 50.0] + [float(v) for v in rng.uniform(0, 100, 12)]:
            i, j, gm = audit.percentile_plan(n, pct)
            got = audit.lerp_f32(x[i], x[j], gm)
            assert np.float32(np.percentile(x, pct)).view(np.uint32) == got.view(np.uint32), (n, pct)


def test_robust_metrics_arguments():
    with pytest.raises(ValueError):
        audit.compute_robust_metrics(np.zeros(0, np.float32), np.zeros(0, np.float32))
    with pytest.raises(ValueError):
        audit.compute_robust_metrics(np.zeros(3, np.float32), np.zeros(3, np.float32), winsorize_pct=120.0)


def test_ops_refuse_host_tensors():
    a = torch.zeros(10)
    with pytest.raises(MmgError):
        ops.order_stats(a, [0])
    with pytest.raises(ValueError):
        ops.order_stats(a, [10])
    with pytest.raises(ValueError):
        ops.order_stats(a, list(range(9)))
    with pytest.raises(Exception):
        ops.split_membership(torch.zeros(4, dtype=torch.int64), *(torch.zeros(4, dtype=torch.bool),) * 3, 1)


def test_c_abi_argument_errors_without_a_gpu():
    from mmgnn import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    rk = (ctypes.c_int64 * 9)(*range(9))
    nul = ctypes.c_void_p(None)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.mmg_order_stats(p, nul, 0, rk, 1, p, p, p, 1 << 20, nul) == -1                 # n = 0
    assert lib.mmg_order_stats(p, nul, 10, rk, 9, p, p, p, 1 << 20, nul) == -1                # 9 ranks
    rk2 = (ctypes.c_int64 * 1)(10)
    assert lib.mmg_order_stats(p, nul, 10, rk2, 1, p, p, p, 1 << 20, nul) == -1               # rank >= n
    assert lib.mmg_order_stats(p, nul, 10, rk, 1, p, p, p, 16, nul) == -3                     # workspace
    assert lib.mmg_order_stats_ws_bytes(10) > 0
    pt = _lib.PercentileT(0, 3, 0.5)
    assert lib.mmg_robust_sums(p, p, 10, p, 2, p, pt, pt, pt, p, p, 1 << 20, nul) == -1       # index 3 of 2
    ok = _lib.PercentileT(0, 1, 0.5)
    assert lib.mmg_robust_sums(p, p, 0, p, 2, p, ok, ok, ok, p, p, 1 << 20, nul) == -1        # n = 0
    assert lib.mmg_robust_sums(p, p, 10, p, 2, p, ok, ok, ok, p, p, 0, nul) == -3
    assert lib.mmg_split_membership(p, p, p, p, -1, 4, p, p, 1 << 20, nul) == -1
    assert lib.mmg_split_membership(p, p, p, p, 4, 1 << 20, p, p, 64, nul) == -3
    assert b"workspace" in lib.mmg_last_error()
