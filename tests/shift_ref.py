"""The cohort-shift tests of mmgnn.shift restated with plain loops and exact arithmetic, on top of rng_ref.  Written from
include/mmgnn_shift.h, never calling the package: the host path and the kernels are compared against THIS.

  labels     key_b(u) = first word of group_words(key(seed, SITE + b), u) << 32 | u;  T[b] = the U_A-th smallest over the
             participating units (sorted Python ints);  u in A iff key_b(u) <= T[b];  replicate 0: group[u] == 1
  tables     pairs of a lab sorted by (value, position); Python ints for n_a, n_b, K_plus, K_minus; Fractions for W and
             the sums (exact), with the sum of the absolute terms and the number of terms for the rounding bound
  finish     the formulas in Python floats (IEEE double, one rounding per operation)
  summary    counting loops
"""
import math
from fractions import Fraction

import numpy as np

import rng_ref

SITE = 0x53484654
F32 = np.float32
NAN = float("nan")


def key_of(seed, b, u):
    w0, _ = rng_ref.group_words(rng_ref.key(seed, SITE + b), np.array([u], dtype=np.uint64))
    return (int(w0[0]) << 32) | int(u)


def thresholds(group, replicates, seed):
    """-> (T list of Python ints [replicates + 1], (U, U_A, status))"""
    part = [u for u, g in enumerate(group) if g <= 1]
    U, UA = len(part), sum(1 for g in group if g == 1)
    if not 1 <= UA < U:
        return [0] * (replicates + 1), (U, UA, 1)
    return [0] + [sorted(key_of(seed, b, u) for u in part)[UA - 1] for b in range(1, replicates + 1)], (U, UA, 0)


def in_a(seed, b, u, group, T):
    return group[u] == 1 if b == 0 else key_of(seed, b, u) <= T[b]


def kept_pairs(value, seg, unit, group, n_seg):
    """-> (per lab the list of (value float32 with -0.0 as +0.0, position, unit) sorted by (value, position), dropped [4])"""
    dropped = [0, 0, 0, 0]
    labs = [[] for _ in range(n_seg)]
    for i, (v, s, u) in enumerate(zip(value, seg, unit)):
        v, s, u = F32(v), int(s), int(u)
        if not 0 <= s < n_seg:
            dropped[0] += 1
        elif not 0 <= u < len(group):
            dropped[1] += 1
        elif not math.isfinite(v):
            dropped[2] += 1
        elif group[u] > 1:
            dropped[3] += 1
        else:
            labs[s].append((float(v) + 0.0, i, u))
    return [sorted(p) for p in labs], dropped


def tables(value, seg, unit, group, n_seg, replicates, seed, T):
    """-> counts int64 [R + 1, n_seg, 4], exact float64 [R + 1, n_seg, 5] (the exact sums rounded once), mag (the sums of
    the absolute terms), nterm int64 [n_seg, 5] (the number of terms of every sum: label independent), dropped"""
    labs, dropped = kept_pairs(value, seg, unit, group, n_seg)
    R1 = replicates + 1
    counts = np.zeros((R1, n_seg, 4), np.int64)
    exact, mag = np.zeros((R1, n_seg, 5)), np.zeros((R1, n_seg, 5))
    nterm = np.zeros((n_seg, 5), np.int64)
    for s, pairs in enumerate(labs):
        m = len(pairs)
        ends = [j for j in range(m) if j == m - 1 or pairs[j + 1][0] != pairs[j][0]]
        nterm[s] = [max(len(ends) - 1, 0), m, m, m, m]
        for r in range(R1):
            lab = [in_a(seed, r, u, group, T) for _, _, u in pairs]
            n_a = sum(lab)
            n_b = m - n_a
            kp = km = 0
            c_a = c_b = 0
            W = Wm = Fraction(0)
            S = [Fraction(0)] * 4
            M = [Fraction(0)] * 4
            nxt = 0
            for j, (v, _, _) in enumerate(pairs):
                a = lab[j]
                c_a, c_b = c_a + a, c_b + (not a)
                fv = Fraction(v)
                k = 0 if a else 1
                S[k] += fv
                S[2 + k] += fv * fv
                M[k] += abs(fv)
                M[2 + k] += fv * fv
                if nxt < len(ends) and j == ends[nxt]:
                    nxt += 1
                    d = c_a * n_b - c_b * n_a
                    kp, km = max(kp, d), max(km, -d)
                    if j < m - 1:
                        W += abs(d) * (Fraction(pairs[j + 1][0]) - fv)
                        Wm += abs(d) * (Fraction(pairs[j + 1][0]) - fv)
            counts[r, s] = [n_a, n_b, kp, km]
            exact[r, s] = [float(W), float(S[0]), float(S[1]), float(S[2]), float(S[3])]
            mag[r, s] = [float(Wm), float(M[0]), float(M[1]), float(M[2]), float(M[3])]
    return counts, exact, mag, nterm, np.array(dropped, np.int64)


def stats6(ci, cd, U, UA):
    n_a, n_b, kp, km = (int(x) for x in ci)
    w, sa, sb, qa, qb = (float(x) for x in cd)
    na, nb = float(n_a), float(n_b)

    def div(a, b):
        if b == 0.0:
            return NAN if a == 0.0 or a != a else math.copysign(math.inf, a)
        return a / b

    out = [NAN] * 5 + [div(na, float(UA)) - div(nb, float(U - UA))]
    if n_a <= 0 or n_b <= 0:
        return out
    P = float(n_a * n_b)
    D = float(max(kp, km)) / P
    out[0], out[1], out[2] = D, D if kp >= km else -D, w / P
    if n_a >= 2 and n_b >= 2:
        va, vb = (qa - sa * sa / na) / (na - 1.0), (qb - sb * sb / nb) / (nb - 1.0)
        va, vb = va if va > 0.0 else 0.0, vb if vb > 0.0 else 0.0
        num, den = sa / na - sb / nb, math.sqrt((va + vb) / 2.0)
        out[3] = 0.0 if num == 0.0 and den == 0.0 else div(num, den)
    out[4] = D * math.sqrt(P / (na + nb))
    return out


def finish(counts, sums, cohort):
    R1, n_seg = counts.shape[:2]
    out = np.full((R1, n_seg + 1, 6), np.nan)
    for r in range(R1):
        best = NAN
        for s in range(n_seg):
            out[r, s] = stats6(counts[r, s], sums[r, s], int(cohort[0]), int(cohort[1]))
            z = out[r, s, 4]
            if z == z and not best >= z:
                best = z
        out[r, n_seg, 4] = best
    return out


def summary(stats):
    R1, rows = stats.shape[:2]
    n_seg = rows - 1
    out = np.full((rows, 7), np.nan)

    def p_of(x0, xs):
        count = sum(1 for x in xs if x >= x0)
        m = sum(1 for x in xs if x == x)
        return ((1.0 + count) / (1.0 + m) if x0 == x0 else NAN), float(count)

    maxz = [float(stats[b, n_seg, 4]) for b in range(R1)]
    for row in range(n_seg):
        col = lambda f, fn=float: [fn(stats[b, row, f]) for b in range(R1)]      # noqa: E731
        d, w, smd, cov = col(0), col(2), [abs(x) for x in col(3)], [abs(x) for x in col(5)]
        out[row, 0], out[row, 5] = p_of(d[0], d[1:])
        out[row, 1], out[row, 2], out[row, 3] = p_of(w[0], w[1:])[0], p_of(smd[0], smd[1:])[0], p_of(cov[0], cov[1:])[0]
        out[row, 4], out[row, 6] = p_of(float(stats[0, row, 4]), maxz[1:])
    out[n_seg, 4], out[n_seg, 6] = p_of(maxz[0], maxz[1:])
    return out
