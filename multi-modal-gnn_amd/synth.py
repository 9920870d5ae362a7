"""Synthetic hetero-graphs of the eICU shape for benchmarks and scale tests.

scale s: N_P = 1,834*s patients; vocab 50 labs / 114 diagnoses / 100 medications (fixed);
exactly 61,484*s has_lab, 5,421*s has_diagnosis, 15,933*s has_medication edges; no duplicate
(patient, item) pair; has_lab degree ~ clipped Normal(33.5, 12) with ~1.5 % of patients forced to 0..5
labs (exercises the degree gate of src/model.py:312-315 and empty neighbourhoods); Zipf-like item
popularity; edge order lab-major for has_lab (what the reference's parquet yields,
src/preprocess.py:141-147) and patient-major for the other two; edge_attr ~ N(0,1).
Runs on any torch device (generation on the GPU at x100/x1000 takes seconds).
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from .data import HeteroGraph

EICU = dict(patients=1834, labs=50, dx=114, meds=100, e_lab=61484, e_dx=5421, e_med=15933)
MIMIC_LIKE = dict(patients=1834, labs=50, dx=200, meds=100, e_lab=61484, e_dx=5421, e_med=15933)


def _degrees(n, mean, std, lo, hi, total, gen, device, frozen=None):
    d = (torch.randn(n, generator=gen, device=device) * std + mean).round().clamp_(lo, hi).long()
    if frozen is not None:
        d = torch.where(frozen >= 0, frozen, d)
    free = torch.ones(n, dtype=torch.bool, device=device) if frozen is None else frozen < 0
    for _ in range(64):                       # nudge +-1 on random free rows until the total is exact
        diff = int(total - int(d.sum()))
        if diff == 0:
            break
        ok = free & ((d < hi) if diff > 0 else (d > lo))
        idx = torch.nonzero(ok).flatten()
        if idx.numel() == 0:
            raise RuntimeError("cannot reach the requested edge total")
        k = min(abs(diff), idx.numel())
        pick = idx[torch.randperm(idx.numel(), generator=gen, device=device)[:k]]
        d[pick] += 1 if diff > 0 else -1
    if int(d.sum()) != total:
        raise RuntimeError("edge total not reached")
    return d


def _poisson_degrees(n, lam, hi, total, gen, device):
    d = torch.poisson(torch.full((n,), float(lam), device=device), generator=gen).clamp_(0, hi).long()
    for _ in range(64):
        diff = int(total - int(d.sum()))
        if diff == 0:
            break
        ok = (d < hi) if diff > 0 else (d > 0)
        idx = torch.nonzero(ok).flatten()
        k = min(abs(diff), idx.numel())
        pick = idx[torch.randperm(idx.numel(), generator=gen, device=device)[:k]]
        d[pick] += 1 if diff > 0 else -1
    if int(d.sum()) != total:
        raise RuntimeError("edge total not reached")
    return d


def _pick_items(deg, n_items, zipf_a, gen, device, chunk=1 << 18):
    """deg[i] distinct items per row, weighted by popularity (Gumbel top-k). -> (rows, items), row-major."""
    w = 1.0 / torch.arange(1, n_items + 1, device=device, dtype=torch.float32) ** zipf_a
    logw = torch.log(w / w.sum())
    rows, items = [], []
    for s in range(0, deg.numel(), chunk):
        d = deg[s:s + chunk]
        u = torch.rand(d.numel(), n_items, generator=gen, device=device).clamp_(1e-12, 1 - 1e-7)
        score = logw - torch.log(-torch.log(u))
        rank = score.argsort(dim=1, descending=True).argsort(dim=1)
        r, c = torch.nonzero(rank < d[:, None], as_tuple=True)
        rows.append(r + s)
        items.append(c)
    return torch.cat(rows), torch.cat(items)


def make_graph(scale: int = 1, seed: int = 0, device="cpu", shape: Dict = EICU,
               with_reverse: bool = True) -> HeteroGraph:
    device = torch.device(device)
    gen = torch.Generator(device=device).manual_seed(seed)
    P = shape["patients"] * scale
    L, DX, M = shape["labs"], shape["dx"], shape["meds"]
    # ~1.5 % low-connectivity patients with 0..5 labs
    frozen = torch.full((P,), -1, dtype=torch.long, device=device)
    low = torch.rand(P, generator=gen, device=device) < 0.015
    frozen[low] = torch.randint(0, 6, (int(low.sum()),), generator=gen, device=device)
    d_lab = _degrees(P, 33.5, 12.0, 0, L, shape["e_lab"] * scale, gen, device, frozen)
    d_dx = _poisson_degrees(P, shape["e_dx"] / shape["patients"], DX, shape["e_dx"] * scale, gen, device)
    d_med = _poisson_degrees(P, shape["e_med"] / shape["patients"], M, shape["e_med"] * scale, gen, device)

    p_lab, i_lab = _pick_items(d_lab, L, 0.35, gen, device)
    order = torch.sort(i_lab, stable=True).indices            # lab-major, patients ascending inside a lab
    p_lab, i_lab = p_lab[order], i_lab[order]
    p_dx, i_dx = _pick_items(d_dx, DX, 0.8, gen, device)
    p_med, i_med = _pick_items(d_med, M, 0.6, gen, device)

    g = HeteroGraph()
    g["patient"].num_nodes = P
    g["lab"].num_nodes = L
    g["diagnosis"].num_nodes = DX
    g["medication"].num_nodes = M
    ei = torch.stack([p_lab, i_lab]).contiguous()
    ea = torch.randn(ei.shape[1], 1, generator=gen, device=device)
    g["patient", "has_lab", "lab"].edge_index = ei
    g["patient", "has_lab", "lab"].edge_attr = ea
    if with_reverse:
        g["lab", "has_lab_rev", "patient"].edge_index = ei.flip(0).contiguous()
        g["lab", "has_lab_rev", "patient"].edge_attr = ea
    ei = torch.stack([p_dx, i_dx]).contiguous()
    g["patient", "has_diagnosis", "diagnosis"].edge_index = ei
    if with_reverse:
        g["diagnosis", "has_diagnosis_rev", "patient"].edge_index = ei.flip(0).contiguous()
    ei = torch.stack([p_med, i_med]).contiguous()
    g["patient", "has_medication", "medication"].edge_index = ei
    if with_reverse:
        g["medication", "has_medication_rev", "patient"].edge_index = ei.flip(0).contiguous()
    return g


def directed_edges(g) -> int:
    return sum(int(g[et].edge_index.shape[1]) for et in g.edge_types)


def make_lab_events(scale: int = 1, seed: int = 0, device="cpu", events_per_pair: float = 6.0) -> Dict:
    """The raw lab events behind make_graph(scale, seed)'s has_lab edges, generated on `device`.

    Every edge (patient, lab) gets 1 + Poisson(events_per_pair - 1) events: times in whole hours of a week, in minutes
    (many ties inside a pair; ~1e-3 of them missing = INT64_MAX), values lab_loc + lab_spread * N(0, 1) in fp64 with the
    labs' locations spread over two orders of magnitude, ~1e-3 gross outliers (9999) and ~5e-3 NaN.  A few patients
    outside the cohort (ids >= n_patients) get events too, and the rows are shuffled.
    -> dict(patient, lab, value, time: tensors over the events; n_patients, n_labs; edge_index: the graph's has_lab
    edges).  Patient and lab ids are their codes."""
    device = torch.device(device)
    g = make_graph(scale, seed, device)
    ei = g["patient", "has_lab", "lab"].edge_index
    P, L, E = int(g["patient"].num_nodes), int(g["lab"].num_nodes), int(ei.shape[1])
    gen = torch.Generator(device=device).manual_seed(seed + 7919)
    cnt = 1 + torch.poisson(torch.full((E,), float(events_per_pair) - 1.0, device=device), generator=gen).long()
    pair = torch.repeat_interleave(torch.arange(E, device=device), cnt)
    n_out_pat = max(3, P // 600)
    n_out = 20 * n_out_pat
    patient = torch.cat([ei[0][pair], P + torch.randint(0, n_out_pat, (n_out,), generator=gen, device=device)])
    lab = torch.cat([ei[1][pair], torch.randint(0, L, (n_out,), generator=gen, device=device)])
    N = patient.numel()
    loc = 10.0 ** torch.linspace(0.0, 2.0, L, dtype=torch.float64, device=device)[torch.randperm(L, generator=gen, device=device)]
    spread = loc * (0.05 + 0.25 * torch.rand(L, generator=gen, device=device, dtype=torch.float64))
    value = loc[lab] + spread[lab] * torch.randn(N, generator=gen, device=device, dtype=torch.float64)
    u = torch.rand(N, generator=gen, device=device)
    value = torch.where(u < 1e-3, torch.full_like(value, 9999.0), value)
    value = torch.where((u >= 1e-3) & (u < 6e-3), torch.full_like(value, float("nan")), value)
    time = torch.randint(0, 7 * 24, (N,), generator=gen, device=device) * 60
    time = torch.where(torch.rand(N, generator=gen, device=device) < 1e-3,
                       torch.full_like(time, torch.iinfo(torch.int64).max), time)
    order = torch.randperm(N, generator=gen, device=device)
    return {"patient": patient[order].contiguous(), "lab": lab[order].contiguous(), "value": value[order].contiguous(),
            "time": time[order].contiguous(), "n_patients": P, "n_labs": L, "edge_index": ei}


def lab_event_frames(ev: Dict, string_itemid: bool = False):
    """(labs, cohort) frames of make_lab_events' result, as the reference's aggregate_lab_values takes them: SUBJECT_ID,
    ITEMID (the lab code, or "lab_%03d" names), VALUENUM, CHARTTIME (minutes; NaN = missing)."""
    import numpy as np
    import pandas as pd
    t = ev["time"].cpu().numpy()
    miss = t == np.iinfo(np.int64).max
    lab = ev["lab"].cpu().numpy()
    labs = pd.DataFrame({"SUBJECT_ID": ev["patient"].cpu().numpy(),
                         "ITEMID": np.array([f"lab_{i:03d}" for i in range(ev["n_labs"])], dtype=object)[lab]
                         if string_itemid else lab,
                         "VALUENUM": ev["value"].cpu().numpy(),
                         "CHARTTIME": np.where(miss, np.nan, t.astype(np.float64))})
    return labs, pd.DataFrame({"SUBJECT_ID": np.arange(ev["n_patients"], dtype=np.int64)})


CODE_KINDS = {"diagnosis": ("has_diagnosis", "diagnosis"), "medication": ("has_medication", "medication")}


def make_code_events(scale: int = 1, seed: int = 0, device="cpu", kind: str = "diagnosis", tail_codes: int = 2048,
                     events_per_pair: float = 2.5) -> Dict:
    """The raw diagnosis / prescription rows behind make_graph(scale, seed)'s has_diagnosis / has_medication edges.

    Every edge (patient, code) gets 1 + Poisson(events_per_pair - 1) rows.  Beyond the graph's vocabulary lie
    tail_codes rare codes (codes n_vocab .. n_codes - 1) with 1..3 patients each -- the long tail a raw ICD-9 or drug
    vocabulary has, which a min_patient_count of 5 removes again.  A few patients outside the cohort (ids >=
    n_patients) get rows too, and the rows are shuffled.
    -> dict(patient, code: int64 tensors over the rows; n_patients, n_vocab, n_codes; edge_index: the graph's edges).
    Patient and code ids are their codes."""
    if kind not in CODE_KINDS:
        raise ValueError(f'kind must be "diagnosis" or "medication", got {kind!r}')
    device = torch.device(device)
    g = make_graph(scale, seed, device)
    rel, node = CODE_KINDS[kind]
    ei = g["patient", rel, node].edge_index
    P, V, E = int(g["patient"].num_nodes), int(g[node].num_nodes), int(ei.shape[1])
    gen = torch.Generator(device=device).manual_seed(seed + (104729 if kind == "diagnosis" else 130003))
    cnt = 1 + torch.poisson(torch.full((E,), float(events_per_pair) - 1.0, device=device), generator=gen).long()
    pair = torch.repeat_interleave(torch.arange(E, device=device), cnt)
    n_tail_pat = torch.randint(1, 4, (tail_codes,), generator=gen, device=device)
    tail_code = V + torch.repeat_interleave(torch.arange(tail_codes, device=device), n_tail_pat)
    tail_patient = torch.randint(0, P, (tail_code.numel(),), generator=gen, device=device)
    n_out_pat = max(3, P // 600)
    n_out = 20 * n_out_pat
    patient = torch.cat([ei[0][pair], tail_patient, P + torch.randint(0, n_out_pat, (n_out,), generator=gen, device=device)])
    code = torch.cat([ei[1][pair], tail_code, torch.randint(0, V, (n_out,), generator=gen, device=device)])
    order = torch.randperm(patient.numel(), generator=gen, device=device)
    return {"patient": patient[order].contiguous(), "code": code[order].contiguous(), "n_patients": P, "n_vocab": V,
            "n_codes": V + tail_codes, "edge_index": ei}


def code_event_frames(ev: Dict, kind: str = "diagnosis"):
    """(rows, cohort) frames of make_code_events' result, as the reference's process_diagnoses / process_medications
    take them: SUBJECT_ID, HADM_ID (SUBJECT_ID + 100000: one admission per patient) and ICD9_CODE ("%03d" of the code
    modulo 1000 followed by the thousands, so that a tail code collapses onto a 3-character code of the vocabulary) or
    DRUG ("drug%04d 10 mg tablet").  The cohort lists every patient below n_patients."""
    import numpy as np
    import pandas as pd
    if kind not in CODE_KINDS:
        raise ValueError(f'kind must be "diagnosis" or "medication", got {kind!r}')
    code = ev["code"].cpu().numpy()
    sid = ev["patient"].cpu().numpy()
    if kind == "diagnosis":
        names = np.array([f"{c % 1000:03d}{c // 1000}" for c in range(ev["n_codes"])], dtype=object)
    else:
        names = np.array([f"Drug{c:04d} 10 mg Tablet" for c in range(ev["n_codes"])], dtype=object)
    rows = pd.DataFrame({"SUBJECT_ID": sid, "HADM_ID": sid + 100000, "ICD9_CODE" if kind == "diagnosis" else "DRUG": names[code]})
    ids = np.arange(ev["n_patients"], dtype=np.int64)
    return rows, pd.DataFrame({"SUBJECT_ID": ids, "HADM_ID": ids + 100000})
