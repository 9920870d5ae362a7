"""Loop-per-segment reference of the split-conformal tables (mmgnn/conformal.py, csrc/conformal.hip), written from the
definitions: np.sort per segment, Python's math.floor / math.ceil for the ranks, np.median for the shift.  Shares no
code with mmgnn.conformal.  Also the seeded cases the CPU and the GPU tests share (make_case, synthetic)."""
import math

import numpy as np

F32 = np.float32
NEG, POS = F32(-np.inf), F32(np.inf)


def bin_of(d, edges):
    for j in range(len(edges) - 1):
        if edges[j] <= d < edges[j + 1]:
            return j
    return -1


def cell_of(patient, lab, n_labs, deg, edges):
    """-> (cell or None, kind of drop or None)"""
    if not 0 <= lab < n_labs:
        return None, 0
    if not 0 <= patient < len(deg):
        return None, 1
    b = bin_of(float(deg[patient]), edges)
    if b < 0:
        return None, 2
    return int(lab) * (len(edges) - 1) + b, None


def ranks(m, alpha, mode):
    """-> (k_lo or None, k_hi)"""
    if mode == "signed":
        return math.floor((m + 1) * (alpha / 2)), math.ceil((m + 1) * (1 - alpha / 2))
    return None, math.ceil((m + 1) * (1 - alpha))


def segment_stats(keys, alpha, mode, min_count=0):
    """keys: the fp32 keys of ONE segment (no NaN) -> (count, q_lo, q_hi, shift, usable)"""
    x = np.sort(np.asarray(keys, F32))
    m = int(x.size)
    k_lo, k_hi = ranks(m, alpha, mode)
    q_hi = x[k_hi - 1] if k_hi <= m else POS
    if mode == "signed":
        q_lo = x[k_lo - 1] if k_lo >= 1 else NEG
        with np.errstate(invalid="ignore", over="ignore"):
            shift = F32(np.median(x)) if m else F32(0)
        ok = k_lo >= 1 and k_hi <= m
    else:
        q_lo, shift, ok = F32(-q_hi), F32(0), k_hi <= m
    return m, F32(q_lo), F32(q_hi), shift, bool(ok and m >= min_count)


def seg_order_stats(keys, seg, n_seg, alpha, mode, min_count=0):
    groups = [[] for _ in range(n_seg)]
    for k, s in zip(np.asarray(keys, F32), seg):
        if 0 <= s < n_seg and not np.isnan(k):
            groups[int(s)].append(k)
    out = [segment_stats(g, alpha, mode, min_count) for g in groups]
    return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], F32), np.array([o[2] for o in out], F32),
            np.array([o[3] for o in out], F32), np.array([o[4] for o in out], np.int32))


def fit(pred, target, patient, lab, n_labs, deg, edges, alpha, mode, min_count=0):
    """-> (table fp32 [3, n_cells], level [n_cells], n_used [n_cells], dropped [4])"""
    nb = len(edges) - 1
    n_cells = n_labs * nb
    by_cell = [[] for _ in range(n_cells)]
    by_lab = [[] for _ in range(n_labs)]
    everything = []
    dropped = [0, 0, 0, 0]
    pred, target = np.asarray(pred, F32), np.asarray(target, F32)
    for i in range(len(pred)):
        c, kind = cell_of(int(patient[i]), int(lab[i]), n_labs, deg, edges)
        with np.errstate(invalid="ignore", over="ignore"):
            r = F32(target[i] - pred[i])
        k = r if mode == "signed" else F32(abs(r))
        if kind is None and np.isnan(k):
            kind = 3
        if kind is not None:
            dropped[kind] += 1
            continue
        by_cell[c].append(k)
        by_lab[c // nb].append(k)
        everything.append(k)
    table = np.zeros((3, n_cells), F32)
    level, n_used = np.zeros(n_cells, np.int32), np.zeros(n_cells, np.int32)
    s_all = segment_stats(everything, alpha, mode, min_count)
    s_lab = [segment_stats(g, alpha, mode, min_count) for g in by_lab]
    for c in range(n_cells):
        for lv, s in enumerate((segment_stats(by_cell[c], alpha, mode, min_count), s_lab[c // nb], s_all)):
            if s[4]:
                table[:, c], level[c], n_used[c] = (s[1], s[2], s[3]), lv, s[0]
                break
        else:
            table[:, c], level[c], n_used[c] = (NEG, POS, 0), 3, 0
    return table, level, n_used, np.array(dropped, np.int64)


def apply_pairs(pred, patient, lab, n_labs, deg, edges, table, use_shift=False):
    pred = np.asarray(pred, F32)
    point, lower, upper = pred.copy(), np.empty_like(pred), np.empty_like(pred)
    for i in range(len(pred)):
        c, _ = cell_of(int(patient[i]), int(lab[i]), n_labs, deg, edges)
        ql, qh, sh = (NEG, POS, F32(0)) if c is None else table[:, c]
        with np.errstate(invalid="ignore", over="ignore"):
            lower[i], upper[i] = F32(pred[i] + ql), F32(pred[i] + qh)
            if use_shift:
                point[i] = F32(pred[i] + sh)
    return point, lower, upper


def coverage(pred, target, patient, lab, n_labs, deg, edges, table):
    """-> (counts int64 [n_cells + 1, 6]: n, covered, below, above, infinite, dropped; list of the fp32 widths per cell)"""
    n_cells = table.shape[1]
    counts = np.zeros((n_cells + 1, 6), np.int64)
    widths = [[] for _ in range(n_cells + 1)]
    _, lower, upper = apply_pairs(pred, patient, lab, n_labs, deg, edges, table)
    for i in range(len(pred)):
        c, _ = cell_of(int(patient[i]), int(lab[i]), n_labs, deg, edges)
        if c is None:
            counts[n_cells, 5] += 1
            continue
        t = target[i]
        if np.isnan(pred[i]) or np.isnan(t):
            counts[c, 5] += 1
            continue
        counts[c, 0] += 1
        counts[c, 1] += int(lower[i] <= t <= upper[i])
        counts[c, 2] += int(t < lower[i])
        counts[c, 3] += int(t > upper[i])
        if np.isfinite(lower[i]) and np.isfinite(upper[i]):
            widths[c].append(F32(upper[i] - lower[i]))
        else:
            counts[c, 4] += 1
    return counts, widths


def coverage_bound(alpha, m, n_eval, k=5.0):
    """k standard deviations of the coverage measured on n_eval pairs after calibrating on m: the coverage given the
    calibration set is Beta(k_hi - k_lo + 1, .) with variance <= alpha (1 - alpha) / (m + 2), the evaluation count is
    binomial on top."""
    return k * math.sqrt(alpha * (1 - alpha) * (1.0 / (m + 2) + 1.0 / n_eval))


# ---------------------------------------------------------------------------------- shared cases
def make_case(seed=0, n=900, n_labs=5, n_pat=40, special=True):
    """Pairs with empty cells (lab 4 has no pair, lab 3 one), ties, +-inf and NaN residuals, a degree outside the bins
    (edges start at 1: degree 0) and indices out of range."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 30, n_pat).astype(np.int32)
    deg[:3] = [0, 5, 6]
    patient = rng.integers(0, n_pat, n).astype(np.int64)
    lab = rng.integers(0, n_labs - 2, n).astype(np.int64)
    pred = rng.standard_normal(n).astype(F32)
    target = (pred + rng.standard_t(4, n) * 0.5).astype(F32)
    if special:
        patient[40:48] = 1                                   # degree 5: in a bin under both sets of edges used here
        target[:40] = pred[:40] + F32(0.25)                  # ties
        target[40:44] = [np.inf, -np.inf, np.nan, np.inf]
        pred[44] = np.nan
        pred[45], target[45] = np.inf, np.inf                # inf - inf: a NaN key
        pred[46:48], target[46:48] = [0.0, -0.0], [0.0, 0.0]  # +-0 keys
        lab[50:53] = [-1, n_labs, 10 ** 9]
        patient[53:56] = [-1, n_pat, 2 ** 40]
        lab[56], patient[56] = -5, -5                        # both: counted under the lab
        lab[60] = n_labs - 2                                 # a cell with one pair
    return dict(pred=pred, target=target, patient=patient, lab=lab, n_labs=n_labs, deg=deg)


def synthetic(seed, m, n_eval, n_labs=12, n_bins=4):
    """Student-t (4 degrees of freedom) residuals with a scale and a bias per cell; every patient has one degree bin."""
    rng = np.random.default_rng(seed)
    edges = [0.0, 2.0, 6.0, 16.0, float("inf")]
    deg = np.array([1, 3, 10, 40], np.int32).repeat(5)       # 20 patients, 5 per bin
    n_cells = n_labs * n_bins
    scale, bias = rng.uniform(0.3, 3.0, n_cells), rng.uniform(-1.0, 1.0, n_cells)

    def draw(per_cell):
        cell = np.arange(n_cells).repeat(per_cell)
        lab, b = cell // n_bins, cell % n_bins
        patient = b * 5 + rng.integers(0, 5, cell.size)
        pred = rng.standard_normal(cell.size).astype(F32)
        target = (pred + bias[cell] + scale[cell] * rng.standard_t(4, cell.size)).astype(F32)
        order = rng.permutation(cell.size)
        return pred[order], target[order], lab[order].astype(np.int64), patient[order].astype(np.int64)

    return edges, deg, draw(m), draw(n_eval)
