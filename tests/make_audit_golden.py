#!/usr/bin/env python3
"""Generate tests/golden/audit_small.npz by running the REFERENCE's own audit_leakage functions (build container only).

Runs only where a checkout of the reference exists (its root in MMGNN_REFERENCE); nothing of it is copied.  torch_geometric is provided by
oracle/pyg_min.py, the graphs by oracle/fixtures.py.  Stored (data only):
  holdout masks (train / val / test, packed) of PatientHoldoutSplitter(seed 42) for a 300-patient graph and for the
  eICU-size graph (61,484 has_lab edges), with its patient counts;
  audit_patient_leakage on both graphs for the reference's EdgeMasker split and for the holdout split;
  compute_robust_metrics on fixed arrays: random, heavy ties, all equal, a NaN, n = 1, n = 2, another winsorize_pct.

Usage:  MMGNN_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/make_audit_golden.py
"""
import json
import logging
import os
import sys

sys.dont_write_bytecode = True

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ["MMGNN_REFERENCE"]
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import fixtures as fx  # noqa: E402
from oracle import pyg_min  # noqa: E402

pyg_min.install_as_torch_geometric()
sys.path.insert(0, os.path.join(REF, "src"))
logging.disable(logging.CRITICAL)

import audit_leakage as ref_audit  # noqa: E402
import train as ref_train  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "audit_small.npz")
GRAPHS = {"small": (300, 12, 15, 10), "eicu": (1834, 50, 114, 100)}


def robust_cases():
    rng = np.random.default_rng(7)
    t = rng.standard_normal(4000).astype(np.float32)
    cases = {
        "random": (t, (t + 0.4 * rng.standard_normal(4000) + 0.05 * rng.standard_cauchy(4000)).astype(np.float32), 5.0),
        "ties": (np.round(t, 1).astype(np.float32), np.round(t + rng.integers(-3, 4, 4000) * 0.25, 1).astype(np.float32),
                 5.0),
        "equal": (np.full(257, 1.5, np.float32), np.full(257, 2.0, np.float32), 5.0),
        "nan": (t[:100].copy(), np.where(np.arange(100) == 37, np.float32(np.nan), t[:100] + 0.3).astype(np.float32), 5.0),
        "n1": (np.array([0.7], np.float32), np.array([-0.2], np.float32), 5.0),
        "n2": (np.array([0.7, -1.1], np.float32), np.array([0.1, 0.4], np.float32), 5.0),
        "pct10": (t[:999].copy(), (t[:999] * 0.8 + 0.1).astype(np.float32), 10.0),
    }
    return cases


def main():
    arrays, meta = {}, {"graphs": {}, "robust": {}}
    for name, shape in GRAPHS.items():
        g = fx.graph_from_frames(fx.det_frames(*shape))
        ei = g["patient", "has_lab", "lab"].edge_index
        hs = ref_audit.PatientHoldoutSplitter(g, 0.7, 0.15, 0.15, seed=42)
        em = ref_train.EdgeMasker(g, 0.7, 0.15, 0.15, mask_fraction=0.2, seed=42)
        for split in ("train", "val", "test"):
            arrays[f"{name}_holdout_{split}"] = np.packbits(getattr(hs, f"{split}_mask").numpy())
        arrays[f"{name}_edges"] = np.array(ei.shape[1])
        edge_rep = ref_audit.audit_patient_leakage(ei, em.train_mask, em.val_mask, em.test_mask)
        hold_rep = ref_audit.audit_patient_leakage(ei, hs.train_mask, hs.val_mask, hs.test_mask)
        meta["graphs"][name] = {"shape": shape, "num_patients": hs.num_patients,
                                "n_train_patients": len(hs.train_patients), "n_val_patients": len(hs.val_patients),
                                "n_test_patients": len(hs.test_patients), "edge_level": edge_rep, "holdout": hold_rep}
    for name, (yt, yp, pct) in robust_cases().items():
        arrays[f"robust_{name}_true"] = yt
        arrays[f"robust_{name}_pred"] = yp
        with np.errstate(all="ignore"):
            meta["robust"][name] = ref_audit.compute_robust_metrics(yt, yp, winsorize_pct=pct)
    np.savez_compressed(OUT, __meta__=np.array(json.dumps(meta)), **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
