"""Plain-loop reference of the stacked recalibration (mmgnn/stacking.py; include/mmgnn_stack.h): per-cell lists of
pairs, exact sums through math.fsum, the systems solved by numpy.linalg.solve on float64 -- and the same systems in
80-bit numpy.longdouble, the yardstick of the solver's accuracy.  Nothing here imports the package."""
import math

import numpy as np

F32 = np.float32
M32 = 0xFFFFFFFF
ST_SITE = 0x53544B31
PIVOT_REL = 1e-10
EDGES3 = [0.0, 6.0, 16.0, float("inf")]


# ---------------------------------------------------------------------------------- the RNG, on Python integers
def mix32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def rng_key(seed, site):
    seed &= 0xFFFFFFFFFFFFFFFF
    h = mix32((seed & M32) ^ 0x9E3779B9)
    return mix32(h ^ (seed >> 32) ^ ((site * 0x632BE5AB) & M32))


def fold_of(patient, folds, seed):
    """the first word of mmg_rng_group(key, patient) for a patient below 2^32, mod folds"""
    return mix32(rng_key(seed, ST_SITE) ^ int(patient)) % folds if folds > 1 else 0


# ---------------------------------------------------------------------------------- cells
def cell_of(patient, lab, n_labs, deg, edges):
    """-> (cell, -1) or (-1, drop kind 0 .. 2)"""
    if not 0 <= lab < n_labs:
        return -1, 0
    if not 0 <= patient < len(deg):
        return -1, 1
    d = float(deg[patient])
    for j in range(len(edges) - 1):
        if edges[j] <= d < edges[j + 1]:
            return lab * (len(edges) - 1) + j, -1
    return -1, 2


def n_fields(K):
    return (K + 1) * (K + 2) // 2 + K + 2


def pair_terms(fs, t):
    """the F terms of one pair as Python floats: products of two fp32 values, exact in double"""
    phi = [1.0] + [float(f) for f in fs]
    t = float(t)
    out = [phi[a] * phi[b] for a in range(len(phi)) for b in range(a, len(phi))]
    return out + [p * t for p in phi] + [t * t]


def cell_lists(c, edges, folds=1, seed=0):
    """-> (lists[fold][cell] = [(features.., target)] in input order, dropped [4])"""
    nb = len(edges) - 1
    lists = [[[] for _ in range(c["n_labs"] * nb)] for _ in range(folds)]
    dropped = [0, 0, 0, 0]
    for i in range(len(c["target"])):
        cell, kind = cell_of(int(c["patient"][i]), int(c["lab"][i]), c["n_labs"], c["deg"], edges)
        vals = [f[i] for f in c["feats"]] + [c["target"][i]]
        if kind < 0 and any(math.isnan(float(v)) for v in vals):
            kind = 3
        if kind >= 0:
            dropped[kind] += 1
            continue
        lists[fold_of(c["patient"][i], folds, seed)][cell].append(tuple(vals))
    return lists, np.array(dropped, np.int64)


def fsum_sums(c, edges, folds=1, seed=0):
    """-> (sums float64 [folds, n_cells, F]: every sum exact and rounded once; mags: the same of the |terms|; dropped)"""
    lists, dropped = cell_lists(c, edges, folds, seed)
    F = n_fields(len(c["feats"]))
    sums = np.zeros((folds, len(lists[0]), F))
    mags = np.zeros_like(sums)
    for fo, row in enumerate(lists):
        for cell, pairs in enumerate(row):
            terms = [pair_terms(p[:-1], p[-1]) for p in pairs]
            for f in range(F):
                sums[fo, cell, f] = math.fsum(x[f] for x in terms)
                mags[fo, cell, f] = math.fsum(abs(x[f]) for x in terms)
    return sums, mags, dropped


# ---------------------------------------------------------------------------------- systems
def system(S, K, ridge):
    """sums [F] -> (A [P, P], rhs [P], m) in float64, formed as the header forms them"""
    P = K + 1
    G, q = np.zeros((P, P)), 0
    for a in range(P):
        for b in range(a, P):
            G[a, b] = G[b, a] = S[q]
            q += 1
    rhs = np.array(S[q:q + P], np.float64)
    A = G.copy()
    rhs[1] = rhs[1] + np.float64(ridge) * G[1, 1]
    for a in range(P):
        A[a, a] = G[a, a] + np.float64(ridge) * G[a, a]
    return A, rhs, float(G[0, 0])


def pivots_pass(A):
    """the header's Cholesky on Python floats: every pivot above PIVOT_REL * A_ii?"""
    P = A.shape[0]
    L = [[0.0] * P for _ in range(P)]
    for i in range(P):
        for j in range(i + 1):
            s = float(A[i, j])
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            if j < i:
                L[i][j] = s / L[j][j]
            else:
                if not s > PIVOT_REL * float(A[i, i]):
                    return False
                L[i][i] = math.sqrt(s)
    return True


def solve_ld(A, rhs):
    """Gaussian elimination with partial pivoting in numpy.longdouble (80-bit on x86)"""
    P = A.shape[0]
    M = np.concatenate([A.astype(np.longdouble), rhs.astype(np.longdouble)[:, None]], axis=1)
    for i in range(P):
        p = i + int(np.argmax(np.abs(M[i:, i])))
        M[[i, p]] = M[[p, i]]
        for r in range(i + 1, P):
            M[r] = M[r] - M[i] * (M[r, i] / M[i, i])
    w = np.zeros(P, np.longdouble)
    for i in range(P - 1, -1, -1):
        w[i] = (M[i, P] - (M[i, i + 1:P] * w[i + 1:]).sum()) / M[i, i]
    return w


def training_sums(sums):
    folds = sums.shape[0]
    rows = []
    for jo in range(folds + 1 if folds > 1 else 1):
        t = np.zeros(sums.shape[1:])
        for fo in range(folds):
            if folds == 1 or fo != jo:
                t = t + sums[fo]
        rows.append(t)
    return np.stack(rows)


def solve(sums, n_labs, n_bins, K, ridge, min_count, solver=None):
    """The three levels and the fallback with plain loops -> (coef [folds_out, n_cells, K + 1], level, n_used, the
    usable systems taken [(A, rhs)] in (fold-out, cell) order).  solver: (A, rhs) -> w, default numpy.linalg.solve."""
    solver = solver or (lambda A, r: np.linalg.solve(A, r))
    T = training_sums(sums)
    fo_n, n_cells = T.shape[0], n_labs * n_bins
    need = max(int(min_count), K + 2)
    coef = np.zeros((fo_n, n_cells, K + 1))
    level = np.zeros((fo_n, n_cells), np.int32)
    n_used = np.zeros((fo_n, n_cells), np.int32)
    taken = []
    for jo in range(fo_n):
        lab_sums = [sum((T[jo, l * n_bins + b] for b in range(n_bins)), np.zeros(T.shape[2])) for l in range(n_labs)]
        all_sums = sum(lab_sums, np.zeros(T.shape[2]))
        for c in range(n_cells):
            for lv, S in enumerate((T[jo, c], lab_sums[c // n_bins], all_sums)):
                A, rhs, m = system(S, K, ridge)
                if m >= need and pivots_pass(A):
                    coef[jo, c], level[jo, c], n_used[jo, c] = solver(A, rhs), lv, int(m)
                    taken.append((A, rhs))
                    break
            else:
                coef[jo, c, 1], level[jo, c] = 1.0, 3
    return coef, level, n_used, taken


def apply_pairs(c, edges, coef, seed=0, cross=False):
    folds = coef.shape[0] - 1 if coef.shape[0] > 1 else 1
    out = np.zeros(len(c["patient"]), F32)
    for i in range(out.size):
        fs = [f[i] for f in c["feats"]]
        cell, kind = cell_of(int(c["patient"][i]), int(c["lab"][i]), c["n_labs"], c["deg"], edges)
        if kind >= 0:
            out[i] = fs[0]
            continue
        w = coef[fold_of(c["patient"][i], folds, seed) if cross else coef.shape[0] - 1, cell]
        y = np.float64(w[0])
        with np.errstate(all="ignore"):
            for k, f in enumerate(fs):
                y = y + np.float64(w[k + 1]) * np.float64(f)
            out[i] = F32(y)
    return out


# ---------------------------------------------------------------------------------- cases
def make_case(seed=0, n=1500, K=2, n_labs=5, n_pat=40, special=True, lattice=False):
    """Pairs over n_labs labs and n_pat patients of degrees 0 .. 39 (degree 0 lies in no bin of [1, 6, 16, inf)).  special:
    every drop kind, in the order of precedence (a pair with a bad lab AND a NaN counts as a bad lab).  lattice: small
    integer values, so that every partial sum is exact in any order."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, 40, n_pat).astype(np.int32)
    deg[:3] = [0, 6, 16]                                     # in no bin of EDGES1 / on the two inner edges
    patient, lab = rng.integers(0, n_pat, n), rng.integers(0, n_labs, n)
    if lattice:
        t = rng.integers(-8, 9, n).astype(F32)
        feats = [rng.integers(-8, 9, n).astype(F32) for _ in range(K)]
    else:
        t = rng.standard_normal(n).astype(F32)
        feats = [(0.4 * t + 0.3 * k + 0.6 * rng.standard_normal(n)).astype(F32) for k in range(K)]
    if special and n >= 40:
        lab[:4] = [-1, n_labs, -7, n_labs + 3]
        feats[0][0] = np.nan                                 # counted as a bad lab, not as a NaN
        patient[4:7] = [-1, n_pat, n_pat + 5]
        lab[4] = -2                                          # bad lab before bad patient
        t[5] = np.nan                                        # counted as a bad patient
        patient[7:9] = 0                                     # degree 0
        patient[9:14] = 5                                    # (a patient with a bin)
        t[9], feats[-1][10], feats[0][11] = np.nan, np.nan, np.nan
        feats[0][12], t[13] = np.inf, -np.inf                # kept: only NaN drops
        if lattice:
            feats[0][12], t[13] = F32(3), F32(-2)
    return dict(feats=feats, target=t, patient=patient.astype(np.int64), lab=lab.astype(np.int64), n_labs=n_labs, deg=deg)


def flat_gnn_split(seed=7, n_labs=10, n_pat=400, per_lab=600):
    """A "GNN" that is flat and offset per lab -- 0.3 t + offset_lab + noise -- next to the per-lab mean of a training
    draw: the failure the reference's calibration table shows.  -> (fit half, score half), each a case dict."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, 40, n_pat).astype(np.int32)
    n = n_labs * per_lab
    lab = np.repeat(np.arange(n_labs), per_lab)
    patient = rng.integers(0, n_pat, n)
    mean_lab = rng.standard_normal(n_labs) * 0.5
    offset = rng.standard_normal(n_labs) * 0.4
    t = (mean_lab[lab] + rng.standard_normal(n)).astype(F32)
    gnn = (0.3 * t + offset[lab] + 0.2 * rng.standard_normal(n)).astype(F32)
    lab_mean = (mean_lab + 0.05 * rng.standard_normal(n_labs)).astype(F32)[lab]
    halves = []
    pick = rng.random(n) < 0.5
    for sel in (pick, ~pick):
        halves.append(dict(feats=[gnn[sel], lab_mean[sel]], target=t[sel], patient=patient[sel].astype(np.int64),
                           lab=lab[sel].astype(np.int64), n_labs=n_labs, deg=deg))
    return halves
