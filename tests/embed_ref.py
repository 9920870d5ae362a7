"""Float64 (and 80-bit) restatement of mmgnn.embed for the tests: centre, SVD of the centred matrix, the sign rule,
variance and ratio, projection, numpy.histogram2d, the panel rule -- plus the test cases and the bounds.

BOUNDS (how each was obtained):

* Gram and means -- compared against an ``np.longdouble`` evaluation of the same sums, relative to
  ``sum_i |x_ia - mu_a| |x_ib - mu_b|`` (means: ``sum_i |x_ia| / n``), the largest entry taken.  Allowed: 8 x the distance
  of numpy-float64's own evaluation (``x64.mean(0)``, ``xc.T @ xc``) from that 80-bit evaluation on the same case -- the
  rule the lab-preprocessing sums use.  ``numpy_distances`` computes it on the CPU; ``GRAM_CASES`` records the values it
  gave (numpy 2.x, OpenBLAS).  The column sums of these cases (fewer than 2^13 fp32 values of magnitude about 1 .. 16)
  are exact in float64 in any order, so numpy's distance for the means is the one rounding of the division by n; the
  (2, 4) case is exact throughout (distance 0: the code under test has to be exact there too).
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
}


def gram_case_x(n, D, ld):
    """The case's fp32 rows as a view of an [n, ld] buffer (ld > D: a padded row stride; the padding holds a large
    value no kernel may read into the sums)."""
    buf = np.full((n, ld), 1e6, np.float32)
    buf[:, :D] = make_case(n, D, seed=n + D)
    return buf[:, :D]


@functools.lru_cache(maxsize=None)
def gram80(n, D, ld):
    """80-bit means and centred Gram of the case, and the two denominators -> dict (computed once per case)."""
    x = np.asarray(gram_case_x(n, D, ld), np.longdouble)
    mean = x.sum(axis=0) / np.longdouble(n)
    xc = x - mean
    gram = xc.T @ xc
    a = np.abs(xc).astype(np.float64)
    return {"mean": mean, "gram": gram, "mean_den": np.abs(x).sum(axis=0).astype(np.float64) / n, "gram_den": a.T @ a}


def distances(mean, gram, n, D, ld):
    """(mean distance, Gram distance) of a float64 evaluation from the 80-bit one, in units of the denominators."""
    ref = gram80(n, D, ld)
    dm = np.abs(np.asarray(mean, np.longdouble) - ref["mean"]).astype(np.float64) / ref["mean_den"]
    dg = np.abs(np.asarray(gram, np.longdouble) - ref["gram"]).astype(np.float64) / ref["gram_den"]
    return float(dm.max()), float(dg.max())


def numpy_distances(n, D, ld):
    """numpy-float64's own distance from the 80-bit evaluation: what BOUNDS is 8 x of."""
    x64 = np.asarray(gram_case_x(n, D, ld), np.float64)
    mean = x64.mean(axis=0)
    xc = x64 - mean
    return distances(mean, xc.T @ xc, n, D, ld)


def gram_bounds(n, D, ld):
    return GRAM_CASES[(n, D, ld)]


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
