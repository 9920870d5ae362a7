"""Float64 (and 80-bit) restatement of mmgnn.embed for the tests: centre, SVD of the centred matrix, the sign rule,
variance and ratio, projection, numpy.histogram2d, the panel rule -- plus the test cases and the bounds.

BOUNDS (how each was obtained):

* Gram and means -- compared against an ``np.longdouble`` evaluation of the same sums, relative to
  ``sum_i |x_ia - mu_a| |x_ib - mu_b|`` (means: ``sum_i |x_ia| / n``), the largest entry taken.  Allowed: 8 x the distance
  of numpy-float64's own evaluation (``x64.mean(0)``, ``xc.T @ xc``) from that 80-bit evaluation on the same case -- the
  rule the lab-preprocessing sums use.  ``numpy_distances`` computes it on the CPU; ``GRAM_CASES`` records the values it
  gave (numpy 2.x, OpenBLAS).  The column sums of the cases of fewer than 2^13 rows (fp32 values of magnitude about
  1 .. 16) are exact in float64 in any order, so numpy's distance for the means is the one rounding of the division by
  n; the (2, 4) case is exact throughout (distance 0: the code under test has to be exact there too).  The bounds of a
  case also hold with columns removed (the non-finite test): an element's sums do not involve the other columns.
* Row projection through the C entry point (``project_ratio``) -- per element
  ``|out - ref| <= 2^-24 |ref| + (D + 8) 2^-53 A`` against the 80-bit ``ref = scale_c sum_d (x_d - mean_d) comps_cd``
  and ``A``, the same sum over absolute values: derived from the arithmetic, no eigenvector in it.
* Projection -- per element ``|out - ref| <= 2^-23 max|ref column|``: one fp32 rounding of an fp64 sum (2^-24 of the
  element) plus as much again for the eigenvector perturbation.  Only valid when the leading eigenvalues are well
  separated: ``assert_gaps`` is asserted first by every test that uses it.
* Components 1e-12 absolute, explained variance and ratio 1e-12 relative, under the same gap assertion.
"""
from __future__ import annotations

import functools

import numpy as np

PROJ_REL = 2.0 ** -23
COMP_ABS = 1e-12
VAR_REL = 1e-12
GAP_REL = 1e-3
BOUND_FACTOR = 8.0

# eight planted singular values for the k = 8 cases (make_case's default four leave components 5.. 8 in the noise, where
# no gap separates them): squares 256 .. 4, every gap at least 4 = 1.6e-2 of the largest
SV8 = (16.0, 12.0, 9.0, 7.0, 5.0, 4.0, 3.0, 2.0)

# the reference's panels, in its order
PANELS = {
    "CBC": ["Hct", "Hgb", "RBC", "WBC x 1000", "platelets x 1000", "MCH", "MCHC", "MCV", "RDW", "MPV"],
    "CMP": ["sodium", "potassium", "chloride", "CO2", "glucose", "BUN", "creatinine", "calcium"],
    "LFT": ["ALT (SGPT)", "AST (SGOT)", "alkaline phos.", "total bilirubin", "direct bilirubin", "total protein",
            "albumin"],
    "Coag": ["PT - INR", "PT", "PTT"],
    "ABG": ["pH", "paCO2", "paO2", "Base Excess", "HCO3"],
}


def make_case(n, D, seed=0, sv=(8, 4, 2, 1), noise=0.05, offset=3.0):
    """fp32 [n, D] data with a planted, well-separated leading spectrum (covariance eigenvalues ~ sv^2, then noise^2) and
    a non-zero mean: the offset is large against the spread, so a one-pass Gram (X^T X - n mu mu^T) visibly loses
    digits."""
    rng = np.random.default_rng(seed)
    r = len(sv)
    z = rng.standard_normal((n, r))
    v = np.linalg.qr(rng.standard_normal((D, r)))[0]
    x = (z * np.asarray(sv, np.float64)) @ v.T + noise * rng.standard_normal((n, D)) + offset
    return x.astype(np.float32)


# ---------------------------------------------------------------------------------------------- PCA
def pca_ref(x, k, whiten=False):
    """sklearn.decomposition.PCA semantics in float64 through the SVD of the centred matrix -> dict."""
    x64 = np.asarray(x, np.float64)
    n = x64.shape[0]
    mean = x64.mean(axis=0)
    xc = x64 - mean
    _, s, vt = np.linalg.svd(xc, full_matrices=False)
    lead = np.argmax(np.abs(vt), axis=1)
    vt = vt * np.sign(vt[np.arange(vt.shape[0]), lead])[:, None]
    var = s * s / (n - 1)
    comps = vt[:k]
    proj = xc @ comps.T
    if whiten:
        proj = proj / np.sqrt(var[:k])
    return {"mean": mean, "components": comps, "explained_variance": var[:k], "explained_variance_ratio": var[:k] / var.sum(),
            "singular_values": s[:k], "projection": proj, "eigenvalues": s * s}


def assert_gaps(eigenvalues, k):
    """The gaps between the first k + 1 eigenvalues exceed GAP_REL of the largest: the components are then determined
    far better than the bounds ask, and a comparison cannot pass or fail by luck."""
    lam = np.concatenate([np.asarray(eigenvalues, np.float64), [0.0]])[:k + 1]
    assert lam.size == k + 1
    gaps = lam[:-1] - lam[1:]
    assert np.all(gaps > GAP_REL * lam[0]), (gaps / lam[0]).tolist()


def check_pca(res, ref, k, projection=None):
    """res (an embed.PCAResult) against pca_ref's dict under BOUNDS; every figure is printed before it is asserted."""
    assert_gaps(ref["eigenvalues"], k)
    d_comp = float(np.abs(res.components - ref["components"]).max())
    d_mean = float(np.abs(res.mean - ref["mean"]).max())
    rel = lambda a, b: float((np.abs(a - b) / np.abs(b)).max())                      # noqa: E731
    d_var = rel(res.explained_variance, ref["explained_variance"])
    d_ratio = rel(res.explained_variance_ratio, ref["explained_variance_ratio"])
    d_sv = rel(res.singular_values, ref["singular_values"])
    p = np.asarray(res.projection if projection is None else projection, np.float64)
    col = np.abs(ref["projection"]).max(axis=0)
    d_proj = float((np.abs(p - ref["projection"]) / col).max())
    print(f"components {d_comp:.3e} mean {d_mean:.3e} var {d_var:.3e} ratio {d_ratio:.3e} sv {d_sv:.3e} "
          f"projection {d_proj:.3e} (of {PROJ_REL:.3e})")
    assert res.components.shape == ref["components"].shape and p.shape == ref["projection"].shape
    assert d_comp <= COMP_ABS and d_mean <= COMP_ABS
    assert d_var <= VAR_REL and d_ratio <= VAR_REL and d_sv <= VAR_REL
    assert d_proj <= PROJ_REL


# ---------------------------------------------------------------------------------------------- Gram and means
# (n, D, ld_x) -> (mean bound, Gram bound) = BOUND_FACTOR x numpy_distances(...), recorded
GRAM_CASES = {
    (2, 4, 4): (BOUND_FACTOR * 0.0, BOUND_FACTOR * 0.0),
    (50, 128, 128): (BOUND_FACTOR * 7.39037447324411e-17, BOUND_FACTOR * 7.225605121683382e-16),
    (63, 64, 64): (BOUND_FACTOR * 7.653487485146695e-17, BOUND_FACTOR * 8.560655385902806e-16),
    (1025, 128, 128): (BOUND_FACTOR * 7.487201743682543e-17, BOUND_FACTOR * 1.2464372745184453e-15),
    (4097, 256, 256): (BOUND_FACTOR * 7.360046588900792e-17, BOUND_FACTOR * 7.490078925395655e-16),
    (3000, 12, 20): (BOUND_FACTOR * 6.589083381949995e-17, BOUND_FACTOR * 7.869222631723643e-16),
    # slabs above their minimum (pca_plan: gram_rows 96, 96, 192; mean_rows 274 in the third), ragged last slabs
    (5000, 256, 256): (BOUND_FACTOR * 7.341794970981506e-17, BOUND_FACTOR * 7.44606677196515e-16),
    (20000, 128, 136): (BOUND_FACTOR * 7.4058397435317e-17, BOUND_FACTOR * 7.212011390733962e-16),
    (140001, 4, 4): (BOUND_FACTOR * 2.531308431770682e-16, BOUND_FACTOR * 8.036104990936348e-16),
    # a ragged last 64-block next to full ones: 4, 16, 4 and 8 columns wide
    (300, 68, 72): (BOUND_FACTOR * 7.360323444126413e-17, BOUND_FACTOR * 1.5311624184694199e-15),
    (33, 80, 80): (BOUND_FACTOR * 8.066394607901991e-17, BOUND_FACTOR * 6.017432923919112e-16),
    (65, 132, 132): (BOUND_FACTOR * 7.430496921308859e-17, BOUND_FACTOR * 7.238503995159488e-16),
    (97, 200, 200): (BOUND_FACTOR * 7.566403741120352e-17, BOUND_FACTOR * 1.0750020027589124e-15),
    # fewer rows than one MFMA step
    (3, 64, 64): (BOUND_FACTOR * 5.856232510070688e-17, BOUND_FACTOR * 1.586770545167059e-16),
}


def gram_case_x(n, D, ld):
    """The case's fp32 rows as a view of an [n, ld] buffer (ld > D: a padded row stride; the padding holds a large
    value no kernel may read into the sums)."""
    buf = np.full((n, ld), 1e6, np.float32)
    buf[:, :D] = make_case(n, D, seed=n + D)
    return buf[:, :D]


def gram80_of(x):
    """80-bit means and centred Gram of the rows x, and the two denominators -> dict."""
    x = np.asarray(x, np.longdouble)
    n = x.shape[0]
    mean = x.sum(axis=0) / np.longdouble(n)
    xc = x - mean
    gram = xc.T @ xc
    a = np.abs(xc).astype(np.float64)
    return {"mean": mean, "gram": gram, "mean_den": np.abs(x).sum(axis=0).astype(np.float64) / n, "gram_den": a.T @ a}


@functools.lru_cache(maxsize=None)
def gram80(n, D, ld):
    """gram80_of the case (computed once per case)."""
    return gram80_of(gram_case_x(n, D, ld))


def distances_from(mean, gram, ref):
    """(mean distance, Gram distance) of a float64 evaluation from the 80-bit one, in units of the denominators."""
    dm = np.abs(np.asarray(mean, np.longdouble) - ref["mean"]).astype(np.float64) / ref["mean_den"]
    dg = np.abs(np.asarray(gram, np.longdouble) - ref["gram"]).astype(np.float64) / ref["gram_den"]
    return float(dm.max()), float(dg.max())


def distances(mean, gram, n, D, ld):
    return distances_from(mean, gram, gram80(n, D, ld))


def numpy_distances(n, D, ld):
    """numpy-float64's own distance from the 80-bit evaluation: what BOUNDS is 8 x of."""
    x64 = np.asarray(gram_case_x(n, D, ld), np.float64)
    mean = x64.mean(axis=0)
    xc = x64 - mean
    return distances(mean, xc.T @ xc, n, D, ld)


def gram_bounds(n, D, ld):
    return GRAM_CASES[(n, D, ld)]


# ---------------------------------------------------------------------------------------------- projection of the rows
# (n, D, k) of the mmg_project_rows cases: n = 1, n not a multiple of 16, two passes of the grid loop with a ragged
# second one (n > 65,536 = 4,096 workgroups x 16 rows), every k parity, the narrowest and the widest D
PROJECT_CASES = [(1, 4, 1), (17, 12, 3), (50, 20, 5), (1000, 128, 7), (1000, 256, 8), (1000, 256, 1), (65537, 16, 8),
                 (70001, 128, 2), (70001, 128, 3), (50, 4, 4)]


@functools.lru_cache(maxsize=None)
def project_case(n, D, k):
    """One case of the row projection -> dict: fp32 rows x (magnitude about 1 .. 16), an fp64 mean near the data's, k
    Gaussian (NOT orthonormal) components, a scale in [0.25, 4] with no power of two in it, and the 80-bit values
    ``sum`` = sum_d (x_d - mean_d) comps_cd and ``abs`` = the same over absolute values, both [n, k] (computed once)."""
    rng = np.random.default_rng(1000 * k + D + n)
    x = make_case(n, D, seed=n + D + k)
    mean = x.astype(np.float64).mean(axis=0) + 0.01 * rng.standard_normal(D)
    comps = rng.standard_normal((k, D))
    scale = rng.uniform(0.25, 4.0, k)
    assert not np.any(np.frexp(scale)[0] == 0.5)
    c80 = comps.astype(np.longdouble).T
    s80 = np.empty((n, k), np.longdouble)
    a80 = np.empty((n, k), np.longdouble)
    for r in range(0, n, 8192):                                      # row chunks: the 80-bit copies stay small
        xc = x[r:r + 8192].astype(np.longdouble) - mean.astype(np.longdouble)
        s80[r:r + 8192] = xc @ c80
        a80[r:r + 8192] = np.abs(xc) @ np.abs(c80)
    for a in (x, mean, comps, scale, s80, a80):
        a.setflags(write=False)
    return {"x": x, "mean": mean, "comps": comps, "scale": scale, "sum": s80, "abs": a80}


def project_ratio(out, case, D, scaled):
    """The largest |out - ref| / (2^-24 |ref| + (D + 8) 2^-53 A) over the elements: ref = scale_c x sum, A = scale_c x
    abs in 80 bits.  The first term is the one fp32 rounding of the result; the second covers the fp64 subtraction,
    the D / 16 fmas of a lane, the four butterfly additions and the scale multiply (each at most 2^-53 of the partial
    sum of absolute values, fewer than D + 8 of them in all)."""
    sc = case["scale"].astype(np.longdouble) if scaled else np.longdouble(1.0)
    ref, A = case["sum"] * sc, case["abs"] * sc
    bound = np.longdouble(2.0 ** -24) * np.abs(ref) + np.longdouble((D + 8) * 2.0 ** -53) * A
    return float((np.abs(np.asarray(out, np.longdouble) - ref) / bound).max())


# ---------------------------------------------------------------------------------------------- grid, panels
def hist2d_ref(y, ex, ey, w=None):
    y = np.asarray(y, np.float32).astype(np.float64)
    h = np.histogram2d(y[:, 0], y[:, 1], bins=(np.asarray(ex, np.float64), np.asarray(ey, np.float64)),
                       weights=None if w is None else np.asarray(w, np.float64))[0]
    return h.astype(np.int64)


def panel_ref(names):
    """index -> the LAST panel (in the reference's order) with an entry the name contains, case-insensitively."""
    out = {}
    for i, name in (names.items() if isinstance(names, dict) else enumerate(names)):
        panel = "Other"
        for p, entries in PANELS.items():
            if any(e.lower() in name.lower() for e in entries):
                panel = p
        out[int(i)] = panel
    return out
