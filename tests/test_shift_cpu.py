"""The cohort-shift tests on the host (mmgnn/shift.py): the numpy path EQUALS the loop reference of shift_ref.py in every
integer and lies inside the rounding bound of its exact sums, the statistics agree with scipy's, the permutation keeps
the cohort size and a patient's pairs together, the test has its size under the null and finds a shifted lab, and the
binding is derived from the header the library is built from."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import scipy.special
import scipy.stats

import mmgnn  # noqa: F401
from mmgnn import _lib, ops
from mmgnn import shift as sh
import shift_ref as ref

F32 = np.float32
U53 = 2.0 ** -53


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def make_case(n=160, n_seg=5, n_units=23, seed=0, lattice=False, special=True):
    rng = np.random.default_rng(seed)
    v = (rng.integers(-3, 4, n) if lattice else rng.normal(size=n)).astype(F32)
    c = {"value": v, "seg": rng.integers(0, n_seg, n), "unit": rng.integers(0, n_units, n),
         "group": (rng.random(n_units) < 0.4).astype(np.uint8), "n_seg": n_seg}
    c["group"][:3] = (1, 0, 2)                                    # both cohorts, and a unit in neither
    c["seg"][c["seg"] == 3] = 2                                   # lab 3 is empty
    if special and n >= 40:
        c["value"][:4] = (0.0, -0.0, 0.0, -0.0)
        c["seg"][:4] = 0
        c["seg"][6], c["seg"][7] = -1, n_seg                      # lab out of range
        c["unit"][8], c["unit"][9] = -3, n_units                  # unit out of range
        c["unit"][10], c["seg"][10] = n_units, -1                 # both: counted under the lab
        c["value"][11], c["value"][12], c["value"][13] = np.nan, np.inf, -np.inf
        c["unit"][14] = 2                                         # a unit in neither cohort
        c["value"][15], c["unit"][15] = np.nan, 2                 # both: counted under the value
    return c


def tables(c, R, seed, chunk=sh.SHIFT_CHUNK):
    T, cohort = sh.host_thresholds(c["group"], R, seed)
    return (T, cohort) + sh.host_stats(c["value"], c["seg"], c["unit"], c["group"], c["n_seg"], T, seed, chunk=chunk)


# ---------------------------------------------------------------------------------- labels and thresholds
@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 - 1])
@pytest.mark.parametrize("n_units", [2, 3, 10, 257])
def test_thresholds_equal_the_sorted_keys_and_every_replicate_keeps_the_cohort_size(seed, n_units):
    rng = np.random.default_rng(n_units)
    group = rng.integers(0, 3, n_units).astype(np.uint8)
    group[:2] = (1, 0)
    R = 7
    T, cohort = sh.host_thresholds(group, R, seed)
    wT, wc = ref.thresholds(group.tolist(), R, seed)
    assert T.dtype == np.uint64 and [int(t) for t in T] == wT and cohort.tolist() == list(wc) and wc[2] == 0
    part = np.flatnonzero(group <= 1)
    for b in range(1, R + 1):
        keys = sh.unit_keys(seed, b, part)
        assert [int(k) for k in keys] == [ref.key_of(seed, b, int(u)) for u in part]
        assert len(set(keys.tolist())) == part.size, "the keys are all distinct"
        assert int(T[b]) == int(np.partition(keys, wc[1] - 1)[wc[1] - 1])
    labels = sh.host_labels(seed, part, group, T, 0, R)
    assert (labels.sum(axis=1) == wc[1]).all(), "every replicate labels exactly U_A units as A"
    assert same(labels[0], group[part] == 1)


def test_every_pair_of_one_patient_shares_its_label():
    c = make_case(n=300, special=False)
    T, _ = sh.host_thresholds(c["group"], 20, 3)
    lab = sh.host_labels(3, c["unit"], c["group"], T, 0, 20)
    for u in np.unique(c["unit"]):
        col = lab[:, c["unit"] == u]
        assert (col == col[:, :1]).all()
    assert (lab[1:] != lab[:1]).any(), "the replicates relabel"


@pytest.mark.parametrize("group", [[0, 0, 0], [1, 1], [2, 2, 1], [2, 0], []])
def test_a_cohort_without_a_unit_is_a_status_and_an_error(group):
    T, cohort = sh.host_thresholds(np.array(group, np.uint8), 3, 0)
    assert cohort[2] == 1 and not T.any() and ref.thresholds(group, 3, 0)[1][2] == 1
    n = len(group)
    with pytest.raises(ValueError, match="cohort"):
        sh.two_sample(np.zeros(n, F32), np.zeros(n, np.int64), np.arange(n), np.array(group, np.uint8), 1, replicates=3)


# ---------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("lattice", [False, True])
@pytest.mark.parametrize("n", [0, 1, 2, 40, 160])
def test_host_tables_equal_the_loop_and_lie_inside_the_bound_of_the_exact_sums(n, lattice):
    c = make_case(n=n, lattice=lattice)
    R, seed = 5, 4
    for chunk in (sh.SHIFT_CHUNK, 16):                            # a chunk shorter than the labs: only the order changes
        T, cohort, counts, sums, dropped = tables(c, R, seed, chunk)
        wc, exact, mag, nterm, wd = ref.tables(c["value"], c["seg"], c["unit"], c["group"].tolist(), c["n_seg"], R, seed,
                                               [int(t) for t in T])
        assert same(counts, wc) and same(dropped, wd), "n_a, n_b, K_plus, K_minus come from Python ints"
        bound = (nterm[None] + 8) * U53 * mag
        assert (np.abs(sums - exact) <= bound).all()
        assert (counts[..., 2:] >= 0).all() and not counts[:, 3].any() and not sums[:, 3].any()
    if n >= 40:
        in_none = (c["unit"] == 2) & (c["seg"] >= 0) & (c["seg"] < c["n_seg"]) & np.isfinite(c["value"])
        assert dropped.tolist() == [3, 2, 4, int(in_none.sum())] and in_none[14] and not in_none[15]


def test_signed_zeros_are_one_tie_group():
    v = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], F32)
    group = np.array([1, 0], np.uint8)
    unit = np.array([0, 1, 1, 0, 0, 1])
    T, _ = sh.host_thresholds(group, 0, 0)
    counts, sums, _ = sh.host_stats(v, np.zeros(6, int), unit, group, 1, T, 0)
    # sorted: -1 (B) | four zeros (A, B, B, A) | 1 (A): at the three group ends c_a n_b - c_b n_a = -3, -3, 0
    assert counts[0, 0].tolist() == [3, 3, 0, 3] and sums[0, 0, 0] == 6.0
    plus, plus_sums, _ = sh.host_stats(np.where(v == 0, F32(0), v), np.zeros(6, int), unit, group, 1, T, 0)
    assert same(plus, counts) and same(plus_sums, sums)


# ---------------------------------------------------------------------------------- scipy
def _one_lab(rng, lattice):
    n_a, n_b = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    draw = (lambda m: rng.integers(-4, 5, m)) if lattice else (lambda m: rng.normal(size=m))
    return draw(n_a).astype(F32), (draw(n_b) + (0 if lattice else 0.3)).astype(F32)


def test_ks_wasserstein_and_the_kolmogorov_law_against_scipy():
    """ks within 2^-51 absolute (scipy rounds two quotients and a difference of numbers at most 1; the integer form
    rounds two conversions and one quotient).  wasserstein: the (t + 8) 2^-53 bound of the sum plus one rounding of the
    quotient, plus scipy's own distance from the exact value on the same data, measured here."""
    rng = np.random.default_rng(0)
    worst_ks = worst_w = worst_scipy = 0.0
    for i in range(300):
        xa, xb = _one_lab(rng, lattice=i % 2 == 0)
        v = np.concatenate((xa, xb))
        group = np.concatenate((np.ones(xa.size, np.uint8), np.zeros(xb.size, np.uint8)))
        res = sh.two_sample(v, np.zeros(v.size, np.int64), None, group, 1, replicates=0)
        row = res.per_lab.iloc[0]
        ks = scipy.stats.ks_2samp(xa.astype(np.float64), xb.astype(np.float64), method="asymp")
        assert abs(row["ks"] - ks.statistic) <= 2.0 ** -51
        worst_ks = max(worst_ks, abs(row["ks"] - ks.statistic))
        d_plus = scipy.stats.ks_2samp(xa.astype(np.float64), xb.astype(np.float64), alternative="greater").statistic
        d_minus = scipy.stats.ks_2samp(xa.astype(np.float64), xb.astype(np.float64), alternative="less").statistic
        assert abs(row["ks_signed"]) == row["ks"]
        if abs(d_plus - d_minus) > 2.0 ** -50:                  # (a tie of the two maxima: + by the header's rule)
            assert (row["ks_signed"] > 0) == (d_plus > d_minus)
        # exact W1 = integral |F_a - F_b| from Fractions
        xs = sorted(set(v.astype(np.float64).tolist()))
        exact = sum(abs(Fraction(int((xa <= x).sum()), xa.size) - Fraction(int((xb <= x).sum()), xb.size))
                    * (Fraction(y) - Fraction(x)) for x, y in zip(xs[:-1], xs[1:]))
        w_scipy = scipy.stats.wasserstein_distance(xa.astype(np.float64), xb.astype(np.float64))
        d_scipy = abs(Fraction(w_scipy) - exact)
        t = len(xs) - 1
        bound = (t + 8 + 1) * U53 * float(exact)
        assert abs(Fraction(float(row["wasserstein"])) - exact) <= bound
        assert abs(row["wasserstein"] - w_scipy) <= bound + float(d_scipy)
        if exact:
            worst_w = max(worst_w, float(abs(Fraction(float(row["wasserstein"])) - exact) / exact) / U53)
            worst_scipy = max(worst_scipy, float(d_scipy / exact) / U53)
        z = row["ks"] * math.sqrt(xa.size * xb.size / (xa.size + xb.size))
        assert abs(row["p_asymptotic"] - scipy.special.kolmogorov(z)) <= 1e-12
    print(f"ks: at most {worst_ks / U53:.3g} * 2^-53 from scipy; wasserstein: at most {worst_w:.3g} * 2^-53 relative from "
          f"the exact value (scipy: {worst_scipy:.3g})")
    for z in np.concatenate((np.linspace(0, 4, 401), [1e-3, 0.04, 0.2, 0.999999, 1.0, 1.000001, 6, 50])):
        assert abs(sh.kolmogorov_sf(z) - scipy.special.kolmogorov(z)) <= 1e-12, z
    assert math.isnan(sh.kolmogorov_sf(float("nan")))


# ---------------------------------------------------------------------------------- finish and summary
def test_finish_and_summary_equal_the_loop_on_every_branch():
    c = make_case(n=160, lattice=True)
    T, cohort, counts, sums, _ = tables(c, 12, 2)
    extra_i = np.array([[0, 0, 0, 0], [3, 0, 0, 0], [1, 1, 1, 0], [1, 5, 0, 5], [4, 4, 0, 0]], np.int64)
    extra_d = np.array([[0, 0, 0, 0, 0], [0, 1.5, 0, 2, 0], [1.0, 2, 1, 4, 1], [2.0, 1, 5, 1, 5],
                        [0, 4, 4, 4, 4]], np.float64)         # empty; one cohort; n < 2: smd NaN; n_a = 1; zero variance and difference
    counts = np.concatenate((counts, np.broadcast_to(extra_i, (13, 5, 4))), axis=1)
    sums = np.concatenate((sums, np.broadcast_to(extra_d, (13, 5, 5))), axis=1)
    got, want = sh.host_finish(counts, sums, cohort), ref.finish(counts, sums, cohort)
    assert same(got, want)
    k = c["n_seg"]
    assert np.isnan(got[0, k, :5]).all() and np.isnan(got[0, k + 1, :5]).all() and not np.isnan(got[0, k + 1, 5])
    assert np.isnan(got[0, k + 2, 3]) and got[0, k + 2, 0] == 1 and np.isnan(got[0, k + 3, 3]) and got[0, k + 3, 1] == -1
    assert got[0, k + 4, 3] == 0 and got[0, k + 4, 0] == 0
    assert np.isnan(got[:, -1, [0, 1, 2, 3, 5]]).all() and same(got[:, -1, 4], np.nanmax(got[:, :-1, 4], axis=1))
    gs, ws = sh.host_summary(got), ref.summary(got)
    assert same(gs, ws)
    assert np.isnan(gs[k, :3]).all() and gs[k, 5] == 0 and np.isnan(gs[-1, [0, 1, 2, 3, 5]]).all()
    all_nan = np.full((4, 3, 6), np.nan)
    assert same(sh.host_summary(all_nan), ref.summary(all_nan)) and np.isnan(sh.host_finish(
        np.zeros((2, 2, 4), np.int64), np.zeros((2, 2, 5)), cohort)[:, 2, 4]).all()


# ---------------------------------------------------------------------------------- validity and power
def test_the_permutation_test_has_its_size_under_the_null():
    """400 seeded null data sets, 1 lab, 60 + 60 patients with a patient effect, 99 replicates: a permutation test is
    exact, so P(p <= 0.1) <= 0.1; the observed share may exceed it by 3 standard errors: 0.1 + 3 sqrt(0.1 * 0.9 / 400)."""
    hits = 0
    for i in range(400):
        rng = np.random.default_rng(1000 + i)
        per = rng.integers(1, 5, 120)
        unit = np.repeat(np.arange(120), per)
        v = (np.repeat(rng.normal(size=120), per) + rng.normal(0, 0.5, unit.size)).astype(F32)
        group = np.zeros(120, np.uint8)
        group[rng.permutation(120)[:60]] = 1
        t = sh.shift_tables(v, np.zeros(unit.size, np.int64), unit, group, 1, replicates=99, seed=i)
        hits += t["summary"][0, 0] <= 0.1
    print("share of null data sets with p_ks <= 0.1:", hits / 400)
    assert hits / 400 <= 0.1 + 3 * math.sqrt(0.1 * 0.9 / 400)


POWER_SEED = 0        # the seed of the data and of the replicates for which the numpy path gives the smallest p-value


def test_a_lab_shifted_by_one_standard_deviation_gets_the_smallest_adjusted_p_value():
    rng = np.random.default_rng(POWER_SEED)
    P, L, R = 600, 8, 199
    per = rng.integers(2, 7, P)
    unit = np.repeat(np.arange(P), per)
    labs = rng.integers(0, L, unit.size)
    group = np.zeros(P, np.uint8)
    group[rng.permutation(P)[:300]] = 1
    v = rng.normal(size=unit.size)
    v[(labs == 3) & (group[unit] == 1)] += 1.0
    res = sh.two_sample(v.astype(F32), labs, unit, group, L, replicates=R, seed=POWER_SEED)
    assert res.per_lab["p_adjusted"][3] == 1 / (R + 1) and res.per_lab["p_ks"][3] == 1 / (R + 1)
    assert res.overall["shifted_labs"] == [3] and res.overall["p"] == 1 / (R + 1)
    assert res.overall["n_units"] == P and res.overall["n_units_a"] == 300
    assert res.per_lab["smd"][3] > 0.7 and res.per_lab["ks_signed"][3] < 0, "A lies to the right: F_a < F_b"
    assert list(res.per_lab.columns) == sh.COLUMNS and res.replicates is None


def test_triples_shift_concatenates_the_cohorts_and_offsets_the_patients():
    rng = np.random.default_rng(2)
    a = (rng.integers(0, 30, 200), rng.integers(0, 3, 200), rng.normal(size=200).astype(F32))
    b = (rng.integers(0, 20, 150), rng.integers(0, 3, 150), rng.normal(size=150).astype(F32))
    res = sh.triples_shift(a, b, 3, replicates=20, seed=1)
    na, nb = int(a[0].max()) + 1, int(b[0].max()) + 1
    want = sh.two_sample(np.concatenate((a[2], b[2])), np.concatenate((a[1], b[1])), np.concatenate((a[0], b[0] + na)),
                         np.concatenate((np.ones(na, np.uint8), np.zeros(nb, np.uint8))), 3, replicates=20, seed=1)
    assert res.per_lab.equals(want.per_lab) and res.overall == want.overall
    assert res.per_lab["n_a"].sum() == 200 and res.per_lab["n_b"].sum() == 150

    class Sharded:
        _comm = object()

    with pytest.raises(NotImplementedError):
        sh.triples_shift(a, b, 3, model=Sharded())
    with pytest.raises(NotImplementedError):
        sh.residual_shift(Sharded(), None, None)
    with pytest.raises(NotImplementedError):
        sh.split_shift(None, None, model=Sharded())


def test_split_shift_on_a_host_graph_runs_the_restatement_and_writes_its_file(tmp_path):
    from mmgnn.audit import PatientHoldoutSplitter
    from mmgnn.synth import make_graph
    g = make_graph(1, seed=0)
    res = sh.split_shift(g, PatientHoldoutSplitter(g), a="val", b="test", output_dir=tmp_path, replicates=20)
    assert sorted(os.listdir(tmp_path)) == ["split_shift.csv"]
    assert len(res.per_lab) == int(g["lab"].num_nodes) and 0 < res.overall["n_units_a"] < res.overall["n_units"]
    assert res.overall["n_units"] < int(g["patient"].num_nodes), "the train patients stand aside"
    assert res.dropped["unit_in_no_cohort"] == 0 and 1 / 21 <= res.overall["p"] <= 1


# ---------------------------------------------------------------------------------- refusals
def test_shapes_and_arguments_outside_the_limits_are_refused():
    z, i0, g = np.zeros(1, F32), np.zeros(1, np.int64), np.array([1, 0], np.uint8)
    for n_seg, rep in ((0, 1), (sh.MAX_SEGMENTS + 1, 1), (1, -1), (1, sh.MAX_REPLICATES + 1)):
        with pytest.raises(ValueError):
            sh.shift_tables(z, i0, i0, g, n_seg, rep)
    with pytest.raises(ValueError):
        sh.host_stats(z, np.zeros(2, np.int64), i0, g, 1, np.zeros(1, np.uint64))
    for alpha in (0.0, 1.0, float("nan")):
        with pytest.raises(ValueError):
            sh.two_sample(z, i0, i0, g, 1, replicates=1, alpha=alpha)
    import torch
    from mmgnn import shift_ops
    with pytest.raises(_lib.MmgError, match="device tensor"):               # never the host path behind the kernels' door
        shift_ops.shift_thresholds(torch.zeros(2, dtype=torch.uint8), 3)


# ---------------------------------------------------------------------------------- the binding
def test_the_shift_header_parses_and_names_what_the_library_defines():
    from mmgnn import shift_ops as m
    b = m.BINDING
    assert isinstance(b, _lib.Binding) and b.stem == "shift"
    assert os.path.basename(b.lib_path) == "libmmgnn_shift.so" and os.path.basename(b.header_path) == "mmgnn_shift.h"
    assert (m.DEFINES, m.SIGNATURES, m.PARAMS) == (b.defines, b.signatures, b.params)
    text = re.sub(r"/\*.*?\*/", "", open(b.header_path).read(), flags=re.S)
    assert sorted(re.findall(r"^\s*#\s*define\s+(MMG_\w+)", text, flags=re.M)) == sorted(b.defines) and b.defines
    for name, v in b.defines.items():
        assert type(v) is int and getattr(m, name) == v
    assert m.SHIFT_SITE == sh.SITE_SHIFT == ref.SITE == 0x53484654 and m.SHIFT_CHUNK == sh.SHIFT_CHUNK
    assert m.SHIFT_MAX_REPLICATES == sh.MAX_REPLICATES == 4096 and m.SHIFT_MAX_SEG == sh.MAX_SEGMENTS == 2048
    assert (m.SHIFT_INT_FIELDS, m.SHIFT_SUM_FIELDS, m.SHIFT_STAT_FIELDS, m.SHIFT_SUMMARY_FIELDS, m.SHIFT_DROP_KINDS) == (
        len(sh.INT_FIELDS), len(sh.SUM_FIELDS), len(sh.STAT_FIELDS), len(sh.SUMMARY_FIELDS), len(sh.DROP_KINDS)) == (4, 5, 6, 7, 4)
    assert m.SHIFT_CHUNK >= 1 and m.SHIFT_RB >= 1 and m.SHIFT_COUNTS == 3 and m.SHIFT_OK == 0 != m.SHIFT_BAD_COHORTS
    assert not set(b.signatures) & set(_lib.SIGNATURES)
    assert os.path.exists(b.lib_path), f"{b.lib_path} is not built (make -C multi-modal-gnn_amd/csrc)"
    ctypes.CDLL(_lib.LIB_PATH, mode=ctypes.RTLD_GLOBAL)               # the satellite links against it
    raw = ctypes.CDLL(b.lib_path)
    for sym in b.signatures:
        assert hasattr(raw, sym), sym
    assert sorted(b.signatures) == sorted(f"mmg_shift_{s}" for s in ("thresholds", "stats", "stats_ws_bytes", "finish", "summary"))
    with_ws = [sym for sym, params in b.params.items() if any(p[0] == "ws" for p in params)]
    assert with_ws == ["mmg_shift_stats"]
    for sym in with_ws:
        assert sym + "_ws_bytes" in b.signatures and b.signatures[sym + "_ws_bytes"][0] is ctypes.c_size_t, sym
        assert [p[0] for p in b.params[sym]][-3:] == ["ws", "ws_bytes", "stream"], sym
    for sym, params in b.params.items():
        if not sym.endswith("_ws_bytes"):
            assert params[-1][0] == "stream", sym
    assert sorted(ops._plans(b)) == sorted(b.signatures)
    makefile = open(os.path.join(os.path.dirname(b.lib_path), "csrc", "Makefile")).read()
    assert re.search(r"^SATELLITES = .*\bshift\b", makefile, flags=re.M)
    assert re.search(r"^#\s+shift\s+\S", makefile, flags=re.M), "the Makefile's comment names the library"


def test_the_host_refusals_of_the_library():
    """Every argument check runs on the host: no device is needed (null pointers are refused after the shape)."""
    from mmgnn import shift_ops as m
    lib = m.load()
    err = lambda: _lib.load().mmg_last_error()                                          # noqa: E731
    E_ARG = _lib.MMG_E_ARG
    C_ = m.SHIFT_CHUNK
    assert lib.mmg_shift_stats_ws_bytes(0, 1, 0) > 0
    assert lib.mmg_shift_stats_ws_bytes(10 * C_, 5, 100) >= 10 * C_ * 28 + 10 * 2 * 7 * 8 * 101
    for n, n_seg, R in ((-1, 5, 4), (2 ** 31, 5, 4), (5, 0, 4), (5, 2049, 4), (5, 5, -1), (5, 5, 4097)):
        assert lib.mmg_shift_stats_ws_bytes(n, n_seg, R) == 0

    def thresholds(n_units=10, R=4):
        return lib.mmg_shift_thresholds(None, n_units, R, 0, None, None, None)

    for kw, msg in ((dict(R=-1), b"replicates"), (dict(R=4097), b"replicates"), (dict(n_units=-1), b"units"),
                    (dict(n_units=2 ** 31), b"units"), (dict(), b"null group"), (dict(n_units=0), b"null output")):
        assert thresholds(**kw) == E_ARG and msg in err(), kw

    def stats(ib=8, n=5, n_seg=3, n_units=10, R=4):
        return lib.mmg_shift_stats(None, None, None, ib, n, n_seg, None, n_units, R, 0, None, None, None, None, None, 0, None)

    for kw, msg in ((dict(R=-1), b"replicates"), (dict(R=4097), b"replicates"), (dict(n_seg=0), b"segments"),
                    (dict(n_seg=2049), b"segments"), (dict(ib=2), b"index_bytes"), (dict(n=-1), b"outside [0, 2^31)"),
                    (dict(n=2 ** 31), b"outside [0, 2^31)"), (dict(n_units=-1), b"units"), (dict(), b"null value"),
                    (dict(n=0), b"null group"), (dict(n=0, n_units=0), b"null thresholds")):
        assert stats(**kw) == E_ARG and msg in err(), kw
    assert lib.mmg_shift_finish(None, None, None, 0, 4, None, None) == E_ARG and b"segments" in err()
    assert lib.mmg_shift_finish(None, None, None, 3, 4, None, None) == E_ARG and b"null" in err()
    assert lib.mmg_shift_summary(None, 3, 4097, None, None) == E_ARG and b"replicates" in err()
    assert lib.mmg_shift_summary(None, 3, 4, None, None) == E_ARG and b"null" in err()
