"""Per-lab cohort-shift tests: do two sets of lab values, or of residuals, come from the same distribution, lab by lab?

The guarantees the evaluation side prints rest on it: split-conformal coverage (``mmgnn.conformal``) holds under
exchangeability of the calibration pairs and the new pair, ``mmgnn.stacking`` ships coefficients fitted on one split to
another, and a model trained on one cohort is used on the next.  ``two_sample`` compares cohort A with cohort B in every
lab by four statistics -- the Kolmogorov-Smirnov distance, the Wasserstein-1 distance, the standardised mean difference
and the difference in coverage (pairs per unit) -- and gives each a permutation p-value: the labels are permuted over the
UNITS (patients: the pairs of one patient are not independent; ``units=None`` is the iid test over pairs), which keeps
the size of A.  ``p_adjusted`` is the single-step maxT adjustment over the labs (the maximum of the scaled KS statistic
z over the labs, replicate by replicate).  DESIGN.md section 5, "Cohort shift".

Definitions (this module's numpy functions are the definition, with include/mmgnn_shift.h; ``tests/shift_ref.py`` restates
them with loops):

* labels: replicate 0 is the labelling given; replicate ``b`` puts unit ``u`` in A iff ``key_b(u) <= T[b]``,
  ``key_b(u) = hash(key(seed, SITE_SHIFT + b), u) << 32 | u`` (the project's counter-based RNG group hash, first word),
  ``T[b]`` the ``U_A``-th smallest key over the participating units.
* tables: pairs in (lab, value) order (stable), tie groups of equal values; per (replicate, lab) the exact integers
  ``n_a, n_b, K_plus, K_minus`` and the fp64 sums ``W, S_a, S_b, Q_a, Q_b``, added in the fixed order of the header
  (chunks of ``SHIFT_CHUNK`` sorted pairs, left to right from 0, chunk sums in chunk order).
* finish, summary: the formulas of the header, every operation rounded in float64 on its own.

HIP tensors run the kernels of libmmgnn_shift.so (csrc/shift.hip); numpy inputs (and host tensors) run the float64
restatement below, which is the checker and never a silent substitute for the kernels.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import pandas as pd
import torch

from .bootstrap import _key, _mix32

SITE_SHIFT = 0x53484654
SHIFT_CHUNK = 2048                    # MMG_SHIFT_CHUNK of include/mmgnn_shift.h (tests check the two against each other)
MAX_REPLICATES = 4096
MAX_SEGMENTS = 2048
INT_FIELDS = ("n_a", "n_b", "k_plus", "k_minus")
SUM_FIELDS = ("w", "sum_a", "sum_b", "sumsq_a", "sumsq_b")
STAT_FIELDS = ("ks", "ks_signed", "wasserstein", "smd", "z", "coverage_diff")
SUMMARY_FIELDS = ("p_ks", "p_wasserstein", "p_smd", "p_coverage", "p_adjusted", "count_ks", "count_adjusted")
DROP_KINDS = ("lab_out_of_range", "unit_out_of_range", "non_finite_value", "unit_in_no_cohort")
COLUMNS = ["lab", "n_a", "n_b", "ks", "ks_signed", "wasserstein", "smd", "coverage_diff", "p_ks", "p_wasserstein", "p_smd",
           "p_coverage", "p_adjusted", "p_asymptotic"]
_U32, _U64 = np.uint32, np.uint64


def _is_dev(x) -> bool:
    return torch.is_tensor(x) and x.is_cuda


def _host(x):
    return np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)


def _check_shape(n_seg: int, replicates: int):
    if not 0 <= int(replicates) <= MAX_REPLICATES:
        raise ValueError(f"{replicates} replicates outside [0, {MAX_REPLICATES}]")
    if not 1 <= int(n_seg) <= MAX_SEGMENTS:
        raise ValueError(f"{n_seg} labs outside [1, {MAX_SEGMENTS}]")


# ============================================================================ the numpy restatement
def unit_keys(seed: int, b: int, units) -> np.ndarray:
    """key_b(u), uint64, of the listed units (below 2^31, so the high half of the 64-bit group index is 0)."""
    u = np.asarray(units).astype(_U32)
    h = _mix32(_U32(_key(seed, SITE_SHIFT + int(b))) ^ u)
    return (h.astype(_U64) << _U64(32)) | u.astype(_U64)


def host_thresholds(group, replicates: int, seed: int = 0):
    """mmg_shift_thresholds in numpy -> (T uint64 [replicates + 1], cohort int64 [3]: U, U_A, status)."""
    group = _host(group).reshape(-1).astype(np.uint8)
    if not 0 <= int(replicates) <= MAX_REPLICATES:
        raise ValueError(f"{replicates} replicates outside [0, {MAX_REPLICATES}]")
    if group.size >= 2 ** 31:
        raise ValueError(f"{group.size} units outside [0, 2^31)")
    part = np.flatnonzero(group <= 1)
    U, UA = int(part.size), int(np.count_nonzero(group == 1))
    ok = 1 <= UA < U
    T = np.zeros(int(replicates) + 1, _U64)
    if ok:
        for b in range(1, int(replicates) + 1):
            T[b] = np.partition(unit_keys(seed, b, part), UA - 1)[UA - 1]
    return T, np.array([U, UA, 0 if ok else 1], np.int64)


def host_labels(seed: int, units, group, T, first: int, last: int) -> np.ndarray:
    """bool [last - first + 1, len(units)]: is the unit in A in replicates first .. last?"""
    units = np.asarray(units).astype(np.int64)
    out = np.empty((last - first + 1, units.size), bool)
    for i, b in enumerate(range(first, last + 1)):
        out[i] = (np.asarray(group)[units] == 1) if b == 0 else unit_keys(seed, b, units) <= _U64(T[b])
    return out


def host_stats(value, seg, unit, group, n_seg: int, T, seed: int = 0, chunk: int = SHIFT_CHUNK, rep_block: int = 32):
    """mmg_shift_stats in numpy -> (counts int64 [R + 1, n_seg, 4], sums float64 [R + 1, n_seg, 5], dropped int64 [4]), in
    the documented order."""
    T = np.asarray(T).astype(_U64).reshape(-1)
    R1 = T.size
    _check_shape(n_seg, R1 - 1)
    value = _host(value).reshape(-1).astype(np.float32)
    seg, unit = _host(seg).reshape(-1).astype(np.int64), _host(unit).reshape(-1).astype(np.int64)
    group = _host(group).reshape(-1).astype(np.uint8)
    n, n_units = value.size, group.size
    if seg.size != n or unit.size != n:
        raise ValueError("host_stats: value, seg and unit need the same length")
    bad_s = (seg < 0) | (seg >= n_seg)
    bad_u = (unit < 0) | (unit >= n_units)
    bad_v = ~np.isfinite(value)
    g = np.where(bad_u, 2, group[np.where(bad_u, 0, unit)] if n_units else 2)
    bad_g = g > 1
    dropped = np.array([bad_s.sum(), (~bad_s & bad_u).sum(), (~bad_s & ~bad_u & bad_v).sum(),
                        (~bad_s & ~bad_u & ~bad_v & bad_g).sum()], np.int64)
    keep = np.flatnonzero(~(bad_s | bad_u | bad_v | bad_g))
    v32 = value[keep] + np.float32(0)                               # -0.0 is taken as +0.0
    order = np.lexsort((v32, seg[keep]))                            # stable: ties in ascending pair position
    K, V, Un = seg[keep][order], v32[order].astype(np.float64), unit[keep][order]
    m = K.size
    counts = np.zeros((R1, n_seg, 4), np.int64)
    sums = np.zeros((R1, n_seg, 5))
    if m == 0:
        return counts, sums, dropped
    same_lab = np.concatenate((K[1:] == K[:-1], [False]))
    Vn = np.concatenate((V[1:], [0.0]))
    end = ~(same_lab & (Vn == V))                                   # the last pair of a tie group
    dv = np.where(same_lab, Vn - V, 0.0)                            # 0 inside a group and at the lab's last group
    Q = V * V
    lab_lo = np.searchsorted(K, np.arange(n_seg + 1))
    for r0 in range(0, R1, rep_block):
        r1 = min(r0 + rep_block, R1)
        A = host_labels(seed, Un, group, T, r0, r1 - 1)
        CA = np.cumsum(A, axis=1, dtype=np.int64)
        for s in range(n_seg):
            lo, hi = int(lab_lo[s]), int(lab_lo[s + 1])
            if hi == lo:
                continue
            a = A[:, lo:hi]
            ca = CA[:, lo:hi] - (CA[:, lo - 1:lo] if lo else 0)
            n_a, n_tot = ca[:, -1], hi - lo
            d = ca * n_tot - np.arange(1, n_tot + 1, dtype=np.int64)[None, :] * n_a[:, None]
            e = end[lo:hi]
            counts[r0:r1, s, 0], counts[r0:r1, s, 1] = n_a, n_tot - n_a
            counts[r0:r1, s, 2] = np.maximum(d[:, e].max(axis=1), 0)
            counts[r0:r1, s, 3] = np.maximum((-d[:, e]).max(axis=1), 0)
            terms = (np.where(e[None, :], np.abs(d).astype(np.float64) * dv[None, lo:hi], 0.0),
                     np.where(a, V[None, lo:hi], 0.0), np.where(a, 0.0, V[None, lo:hi]),
                     np.where(a, Q[None, lo:hi], 0.0), np.where(a, 0.0, Q[None, lo:hi]))
            cuts = [lo] + list(range((lo // chunk + 1) * chunk, hi, chunk)) + [hi]
            for f, t in enumerate(terms):
                acc = np.zeros(r1 - r0)
                for p, q in zip(cuts[:-1], cuts[1:]):               # left to right inside a chunk, chunk after chunk
                    acc = acc + np.cumsum(t[:, p - lo:q - lo], axis=1)[:, -1]
                sums[r0:r1, s, f] = acc
    return counts, sums, dropped


def host_finish(counts, sums, cohort) -> np.ndarray:
    """mmg_shift_finish in numpy -> stats float64 [R + 1, n_seg + 1, 6]; row n_seg: the maximum of z in field 4."""
    counts, sums = np.asarray(counts, np.int64), np.asarray(sums, np.float64)
    U, UA = int(cohort[0]), int(cohort[1])
    R1, n_seg = counts.shape[:2]
    n_a, n_b, kp, km = (counts[..., i] for i in range(4))
    w, sa, sb, qa, qb = (sums[..., i] for i in range(5))
    out = np.full((R1, n_seg + 1, 6), np.nan)
    with np.errstate(all="ignore"):
        na, nb = n_a.astype(np.float64), n_b.astype(np.float64)
        P = (n_a * n_b).astype(np.float64)
        D = np.maximum(kp, km).astype(np.float64) / P
        va = (qa - sa * sa / na) / (na - 1.0)
        vb = (qb - sb * sb / nb) / (nb - 1.0)
        va, vb = np.where(va > 0.0, va, 0.0), np.where(vb > 0.0, vb, 0.0)
        num, den = sa / na - sb / nb, np.sqrt((va + vb) / 2.0)
        smd = np.where((num == 0.0) & (den == 0.0), 0.0, num / den)
        smd = np.where((n_a >= 2) & (n_b >= 2), smd, np.nan)
        z = D * np.sqrt(P / (na + nb))
        both = (n_a > 0) & (n_b > 0)
        lab = np.stack([D, np.where(kp >= km, D, -D), w / P, smd, z], axis=-1)
        out[:, :n_seg, :5] = np.where(both[..., None], lab, np.nan)
        out[:, :n_seg, 5] = na / np.float64(UA) - nb / np.float64(U - UA)
        out[:, n_seg, 4] = np.fmax.reduce(out[:, :n_seg, 4], axis=1, initial=np.nan) if n_seg else np.nan
    return out


def host_summary(stats) -> np.ndarray:
    """mmg_shift_summary in numpy -> float64 [n_seg + 1, 7] (SUMMARY_FIELDS)."""
    stats = np.asarray(stats, np.float64)
    rows = stats.shape[1]
    n_seg = rows - 1
    out = np.full((rows, 7), np.nan)
    maxz = stats[:, n_seg, 4]

    def p_of(x0, xb):
        with np.errstate(invalid="ignore"):
            count = int(np.count_nonzero(xb >= x0))
        m = int(np.count_nonzero(~np.isnan(xb)))
        return (np.float64(1.0 + count) / np.float64(1.0 + m) if not np.isnan(x0) else np.nan), float(count)

    for row in range(n_seg):
        x = stats[:, row]
        out[row, 0], out[row, 5] = p_of(x[0, 0], x[1:, 0])
        out[row, 1] = p_of(x[0, 2], x[1:, 2])[0]
        out[row, 2] = p_of(abs(x[0, 3]), np.abs(x[1:, 3]))[0]
        out[row, 3] = p_of(abs(x[0, 5]), np.abs(x[1:, 5]))[0]
        out[row, 4], out[row, 6] = p_of(x[0, 4], maxz[1:])
    out[n_seg, 4], out[n_seg, 6] = p_of(maxz[0], maxz[1:])
    return out


def kolmogorov_sf(z: float) -> float:
    """The limiting Kolmogorov law 2 sum_{k>=1} (-1)^(k-1) exp(-2 k^2 z^2); below z = 1 the same function through its
    theta-function form 1 - sqrt(2 pi) / z * sum_{k>=1} exp(-(2k-1)^2 pi^2 / (8 z^2)), which does not cancel there."""
    z = float(z)
    if math.isnan(z):
        return math.nan
    if z <= 0.0:
        return 1.0
    if z < 1.0:
        t = sum(math.exp(-(2 * k - 1) ** 2 * math.pi ** 2 / (8.0 * z * z)) for k in range(1, 9))
        return min(1.0, max(0.0, 1.0 - math.sqrt(2.0 * math.pi) / z * t))
    return min(1.0, max(0.0, 2.0 * sum((-1.0) ** (k - 1) * math.exp(-2.0 * k * k * z * z) for k in range(1, 12))))


# ============================================================================ the four steps, device or host
def shift_tables(values, labs, units, group, n_labs: int, replicates: int = 1000, seed: int = 0) -> Dict:
    """-> {"T", "cohort", "counts", "sums", "dropped", "stats", "summary"}: HIP tensors run the four calls of
    libmmgnn_shift.so (labs and units both int64 or both int32) and return device tensors; numpy arrays and host tensors
    run the restatement.  Mixing the two is refused."""
    _check_shape(n_labs, replicates)
    given = [x for x in (values, labs, units, group) if x is not None]
    if any(_is_dev(x) for x in given):
        if not all(_is_dev(x) for x in given):
            raise TypeError("shift_tables: every input on the HIP device, or none (no silent host fallback)")
        from . import shift_ops as so
        v = values.reshape(-1).to(torch.float32).contiguous()
        labs = labs.reshape(-1).contiguous()
        units = torch.arange(v.numel(), dtype=labs.dtype, device=v.device) if units is None else units.reshape(-1).contiguous()
        group = group.reshape(-1).to(torch.uint8).contiguous()
        T, cohort = so.shift_thresholds(group, replicates, seed)
        counts, sums, dropped = so.shift_stats(v, labs, units, group, n_labs, T, seed)
        stats = so.shift_finish(counts, sums, cohort)
        return {"T": T, "cohort": cohort, "counts": counts, "sums": sums, "dropped": dropped, "stats": stats,
                "summary": so.shift_summary(stats)}
    v = _host(values).reshape(-1)
    units = np.arange(v.size, dtype=np.int64) if units is None else _host(units)
    T, cohort = host_thresholds(group, replicates, seed)
    counts, sums, dropped = host_stats(v, labs, units, group, n_labs, T, seed)
    stats = host_finish(counts, sums, cohort)
    return {"T": T, "cohort": cohort, "counts": counts, "sums": sums, "dropped": dropped, "stats": stats,
            "summary": host_summary(stats)}


@dataclass
class ShiftResult:
    per_lab: pd.DataFrame
    overall: Dict
    replicates: Optional[Dict] = None
    dropped: Dict[str, int] = field(default_factory=dict)


def two_sample(values, labs, units, group, n_labs: int, replicates: int = 1000, seed: int = 0, alpha: float = 0.05,
               return_replicates: bool = False) -> ShiftResult:
    """Compare cohort A (``group[unit] == 1``) with cohort B (``== 0``; any other value: the unit stands aside) in every
    lab.  ``per_lab``: one row per lab with the columns ``COLUMNS``; ``overall``: the max-z statistic, its permutation
    p-value, the labs with ``p_adjusted <= alpha``, the cohort sizes and the dropped counts; ``replicates``: the tables of
    ``shift_tables`` when asked for (device tensors for device inputs).  ``units=None`` is the iid test: the unit is the
    pair's position and ``group`` has one entry per pair.  ``p_asymptotic`` is the limiting Kolmogorov law of z, for
    comparison only: with dependent pairs per patient the permutation p-values are the ones to act on.  Raises ValueError
    unless both cohorts have a participating unit."""
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError(f"alpha {alpha} outside (0, 1)")
    t = shift_tables(values, labs, units, group, n_labs, replicates, seed)
    cohort = _host(t["cohort"])
    U, UA = int(cohort[0]), int(cohort[1])
    if int(cohort[2]) != 0:
        raise ValueError(f"two_sample: {UA} of the {U} participating units are in cohort A; both cohorts need one")
    counts0, stats0, summ = _host(t["counts"][0]), _host(t["stats"][0]), _host(t["summary"])
    dropped = {k: int(x) for k, x in zip(DROP_KINDS, _host(t["dropped"]).tolist())}
    frame = pd.DataFrame({"lab": np.arange(n_labs), "n_a": counts0[:, 0], "n_b": counts0[:, 1]})
    for k, name in enumerate(STAT_FIELDS):
        if name != "z":
            frame[name] = stats0[:n_labs, k]
    for k, name in enumerate(SUMMARY_FIELDS[:5]):
        frame[name] = summ[:n_labs, k]
    frame["p_asymptotic"] = [kolmogorov_sf(z) for z in stats0[:n_labs, 4]]
    frame = frame[COLUMNS]
    with np.errstate(invalid="ignore"):
        shifted = [int(j) for j in np.flatnonzero(summ[:n_labs, 4] <= alpha)]
    overall = {"max_z": float(stats0[n_labs, 4]), "p": float(summ[n_labs, 4]), "shifted_labs": shifted,
               "alpha": float(alpha), "replicates": int(replicates), "seed": int(seed), "n_units": U, "n_units_a": UA,
               "dropped": dropped}
    return ShiftResult(frame, overall, t if return_replicates else None, dropped)


# ============================================================================ drivers
def _refuse_sharded(model, what: str):
    if model is not None and getattr(model, "_comm", None) is not None:
        raise NotImplementedError(f"{what} on a patient-sharded model (dist.shard_model) is not supported: the forward's "
                                  "collectives need every rank; test with an unsharded model")


def _two_splits(pairs_a, pairs_b, n_pat: int, by_patient: bool):
    """(patient, lab, value) of the two splits -> values, labs, units, group: the unit is the patient (group by patient:
    1 for the patients of a, 0 for those of b, 2 for the rest) or the pair's position."""
    (pa, la, va), (pb, lb, vb) = pairs_a, pairs_b
    if torch.is_tensor(va):
        cat, dev = torch.cat, va.device
        values, labs = cat((va.reshape(-1).float(), vb.reshape(-1).float())), cat((la, lb))
        if by_patient:
            group = torch.full((n_pat,), 2, dtype=torch.uint8, device=dev)
            group[pb] = 0
            group[pa] = 1
            return values, labs, cat((pa, pb)), group
        group = cat((torch.ones(va.numel(), dtype=torch.uint8, device=dev), torch.zeros(vb.numel(), dtype=torch.uint8, device=dev)))
        return values, labs, None, group
    values, labs = np.concatenate((va, vb)).astype(np.float32), np.concatenate((la, lb))
    if by_patient:
        group = np.full(n_pat, 2, np.uint8)
        group[pb] = 0
        group[pa] = 1
        return values, labs, np.concatenate((pa, pb)), group
    return values, labs, None, np.concatenate((np.ones(len(va), np.uint8), np.zeros(len(vb), np.uint8)))


def _write(res: ShiftResult, output_dir, name: str):
    if output_dir is not None:
        output_dir = Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        res.per_lab.to_csv(output_dir / name, index=False)
    return res


def split_shift(graph, masker, a: str = "train", b: str = "test", output_dir=None, model=None, **kw) -> ShiftResult:
    """Compare the lab values of two splits of ``masker``; with ``output_dir`` writes ``split_shift.csv``.  The unit is the
    patient when the masker is a ``PatientHoldoutSplitter``, otherwise the pair.  Runs where the graph lives: a graph on the
    HIP device runs the kernels.  ``model``: only looked at to refuse a patient-sharded one."""
    from .audit import PatientHoldoutSplitter
    from .conformal import _split_pairs
    _refuse_sharded(model, "split_shift")
    sa, sb = _split_pairs(graph, masker, a), _split_pairs(graph, masker, b)
    args = _two_splits((sa[0], sa[1], sa[2]), (sb[0], sb[1], sb[2]), int(graph["patient"].num_nodes),
                       isinstance(masker, PatientHoldoutSplitter))
    return _write(two_sample(*args, n_labs=int(graph["lab"].num_nodes), **kw), output_dir, "split_shift.csv")


def residual_shift(model, graph, masker, a: str = "val", b: str = "test", output_dir=None, **kw) -> ShiftResult:
    """Compare the residuals ``prediction - target`` of two splits; with ``output_dir`` writes ``residual_shift.csv``.  The
    exchangeability check for a ``LabConformal`` or ``LabStacker`` fitted on ``a`` and used on ``b``."""
    from .audit import PatientHoldoutSplitter
    from .conformal import _predict_split
    _refuse_sharded(model, "residual_shift")
    out = []
    for split in (a, b):
        _, pred, y, pi, li = _predict_split(model, graph, masker, split)
        out.append((pi, li, pred - y))
    args = _two_splits(out[0], out[1], int(graph["patient"].num_nodes), isinstance(masker, PatientHoldoutSplitter))
    return _write(two_sample(*args, n_labs=int(graph["lab"].num_nodes), **kw), output_dir, "residual_shift.csv")


def triples_shift(triples_a, triples_b, n_labs: int, model=None, **kw) -> ShiftResult:
    """Two cohorts as (patient, lab, value) triples in ONE lab index space (two databases mapped to the same labs): they
    are concatenated, B's patients offset behind A's, and the unit is the patient.  ``model``: only looked at to refuse a
    patient-sharded one."""
    _refuse_sharded(model, "triples_shift")
    (pa, la, va), (pb, lb, vb) = triples_a, triples_b
    dev = _is_dev(va)
    n_a = int(pa.max()) + 1 if len(pa) else 0
    n_b = int(pb.max()) + 1 if len(pb) else 0
    if dev:
        group = torch.cat((torch.ones(n_a, dtype=torch.uint8, device=va.device), torch.zeros(n_b, dtype=torch.uint8, device=va.device)))
        return two_sample(torch.cat((va.reshape(-1).float(), vb.reshape(-1).float())), torch.cat((la, lb)),
                          torch.cat((pa, pb + n_a)), group, n_labs, **kw)
    pa, la, va, pb, lb, vb = (_host(x).reshape(-1) for x in (pa, la, va, pb, lb, vb))
    group = np.concatenate((np.ones(n_a, np.uint8), np.zeros(n_b, np.uint8)))
    return two_sample(np.concatenate((va, vb)).astype(np.float32), np.concatenate((la, lb)), np.concatenate((pa, pb + n_a)),
                      group, n_labs, **kw)
