"""The patient-cluster bootstrap of mmgnn.bootstrap restated with plain loops, on top of rng_ref.  Written from the
documented algorithm, never calling the package: the host path and the kernels are compared against THIS.

  weights   k_b = key(seed, SITE_BOOT + b);  w0 = the FIRST word of group_words(k_b, u >> 1);
            field = w0 >> 16 if u & 1 else w0 & 0xFFFF;  w = #{j: field >= T[j]};  replicate 0: every weight 1
  sums      per (replicate, segment) the sum of w * term, pairs in input order inside a segment
  metrics   evaluate.metrics_from_sums, copied
  summary   numpy.percentile / mean / std(ddof=1) over the finite replicates
"""
import math

import numpy as np

import rng_ref

SITE_BOOT = 0x424F4F54
T = (24109, 48219, 60273, 64292, 65296, 65497, 65531, 65535)
F32 = np.float32


def weight(seed, b, u):
    if b == 0:
        return 1
    w0, _ = rng_ref.group_words(rng_ref.key(seed, SITE_BOOT + b), np.array([u >> 1], dtype=np.uint64))
    w0 = int(w0[0])
    fld = (w0 >> 16) if (u & 1) else (w0 & 0xFFFF)
    return sum(1 for t in T if fld >= t)


def weights(seed, n_units, replicates):
    """int64 [replicates + 1, n_units]"""
    return np.array([[weight(seed, b, u) for u in range(n_units)] for b in range(replicates + 1)],
                    dtype=np.int64).reshape(replicates + 1, n_units)


def weights_at(seed, units, replicates):
    """int64 [replicates + 1, len(units)]: the weights of the listed units (any values below 2^63), one hash call per
    replicate."""
    units = np.asarray(units, dtype=np.uint64)
    out = np.ones((replicates + 1, units.size), np.int64)
    thr = np.asarray(T, np.uint32)
    for b in range(1, replicates + 1):
        w0, _ = rng_ref.group_words(rng_ref.key(seed, SITE_BOOT + b), units >> np.uint64(1))
        fld = np.where((units & np.uint64(1)) != 0, w0 >> np.uint32(16), w0 & np.uint32(0xFFFF))
        out[b] = (fld[:, None] >= thr[None, :]).sum(1)
    return out


def terms(p, t, pb=None):
    """The additive terms of one pair (float32 inputs) as Python floats, formed as k_seg_metrics forms them."""
    p, t = F32(p), F32(t)
    with np.errstate(all="ignore"):
        e = F32(t - p)
        out = [1.0, float(np.abs(e)), float(e) * float(e), float(t), float(t) * float(t),
               float(np.abs(F32(e / t))) if t != 0 else 0.0, 1.0 if t != 0 else 0.0]
        if pb is not None:
            eb = F32(t - F32(pb))
            out += [float(np.abs(eb)), float(eb) * float(eb), float(np.abs(F32(eb / t))) if t != 0 else 0.0]
    return out


def sums(pred, target, unit, seg, n_units, n_seg, replicates, seed, pred_b=None, want_bound=False):
    """The plain double loop -> (sums [replicates + 1, n_seg, F], dropped [3]) and, on request, per (replicate, segment,
    field) the sum of w * |term| and per segment the number of kept pairs (for the error bound of another order)."""
    F = 7 if pred_b is None else 10
    n = len(pred)
    W = weights(seed, n_units, replicates) if n_units > 0 else np.zeros((replicates + 1, 0), np.int64)
    out = np.zeros((replicates + 1, n_seg, F))
    mag = np.zeros((replicates + 1, n_seg, F))
    count = np.zeros(n_seg, np.int64)
    dropped = np.zeros(3, np.int64)
    kept = []
    for i in range(n):
        s, u = int(seg[i]), int(unit[i])
        vals = [pred[i], target[i]] + ([pred_b[i]] if pred_b is not None else [])
        if s < 0 or s >= n_seg:
            dropped[0] += 1
        elif u < 0 or u >= n_units:
            dropped[1] += 1
        elif any(math.isnan(float(v)) for v in vals):
            dropped[2] += 1
        else:
            kept.append((i, s, u, terms(pred[i], target[i], None if pred_b is None else pred_b[i])))
            count[s] += 1
    for b in range(replicates + 1):
        for i, s, u, tm in kept:
            w = float(W[b, u])
            for f in range(F):
                out[b, s, f] += w * tm[f]
                mag[b, s, f] += w * abs(tm[f])
    return (out, dropped, mag, count) if want_bound else (out, dropped)


def metrics_from_sums(s):
    """evaluate.metrics_from_sums, copied: (mae, rmse, r2, mape)."""
    n, s_abs, s_sq, s_t, s_t2, s_ape, n_nz = (float(s[i]) for i in range(7))
    nan = float("nan")
    if n <= 0:
        return [nan, nan, nan, nan]
    ss_tot = s_t2 - s_t * s_t / n
    if n < 2:
        r2 = nan
    elif s_sq == 0:
        r2 = 1.0
    elif ss_tot > 1e-12 * max(s_t2, 1e-300):
        r2 = 1.0 - s_sq / ss_tot
    else:
        r2 = 0.0
    mape = s_ape / n_nz * 100.0 if n_nz > 0 else nan
    return [s_abs / n, float(np.sqrt(s_sq / n)), r2, mape]


def metrics(sm):
    """sums [R + 1, n_seg, F] -> [R + 1, n_seg + 1, M]; row n_seg: the sums added in segment order."""
    R1, n_seg, F = sm.shape
    M = 4 if F == 7 else 12
    out = np.full((R1, n_seg + 1, M), np.nan)
    for b in range(R1):
        for row in range(n_seg + 1):
            if row < n_seg:
                s = sm[b, row]
            else:
                s = np.zeros(F)
                for j in range(n_seg):
                    s = s + sm[b, j]
            m = metrics_from_sums(s)
            out[b, row, :4] = m
            if F == 10:
                mb = metrics_from_sums([s[0], s[7], s[8], s[3], s[4], s[9], s[6]])
                out[b, row, 4:8] = mb
                out[b, row, 8:] = [x - y for x, y in zip(m, mb)]
    return out


def percents(confidence):
    c = float(confidence)
    return (1.0 - c) / 2.0 * 100.0, (1.0 + c) / 2.0 * 100.0


def summary(mt, confidence):
    """metrics [R + 1, rows, M] -> [rows, M, 7]: estimate, mean, std (ddof 1), lower, upper, n finite, share < 0."""
    _, rows, M = mt.shape
    p_lo, p_hi = percents(confidence)
    out = np.full((rows, M, 7), np.nan)
    for r in range(rows):
        for k in range(M):
            x = mt[1:, r, k]
            x = x[np.isfinite(x)]
            out[r, k, 0], out[r, k, 5] = mt[0, r, k], x.size
            if x.size:
                out[r, k, 1] = np.mean(x)
                out[r, k, 3], out[r, k, 4] = np.percentile(x, p_lo), np.percentile(x, p_hi)
                out[r, k, 6] = np.count_nonzero(x < 0) / x.size
            if x.size > 1:
                out[r, k, 2] = np.std(x, ddof=1)
    return out
