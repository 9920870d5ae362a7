"""The cohort-shift kernels of libmmgnn_shift.so (csrc/shift.hip) against the numpy restatement of mmgnn/shift.py, which
tests/test_shift_cpu.py pins to the loop reference of shift_ref.py: the thresholds EQUAL numpy.partition, the integer
tables EQUAL, every fp64 sum inside the (t + 8) 2^-53 bound of its exact value, finish and summary EQUAL the restatement
on the device's own upstream tables -- at every shape where the kernels take another path -- and the whole is bitwise
repeatable, eagerly and from a hipGraph.

The exact value of a sum is taken in numpy's extended precision (64-bit significand): its own distance from the exact
value, at most 3 (t + 1) 2^-64 of the sum of the absolute terms, is SUBTRACTED from the bound, so passing here implies the
bound against the exact value."""
import numpy as np
import pandas as pd
import pytest
import torch

import mmgnn  # noqa: F401
from mmgnn import ops
from mmgnn import shift as sh
from mmgnn import shift_ops as so
from mmgnn._lib import MmgError
from mmgnn.audit import PatientHoldoutSplitter
from mmgnn.model import build_model
from mmgnn.synth import make_graph
from mmgnn.train import EdgeMasker

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
LD = np.longdouble
C, RB = so.SHIFT_CHUNK, so.SHIFT_RB
U53 = 2.0 ** -53


@pytest.fixture(autouse=True)
def stop_at_a_device_fault():
    """A kernel fault surfaces at the next synchronisation: nothing more is started on the device after one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device fault, stopping the session: {e}", returncode=3)


def same(got, want):
    got, want = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.array_equal(got, want, equal_nan=got.dtype.kind == "f"))


def bits(t):
    return t.contiguous().view(torch.uint8)


def make_case(layout, n_seg, n_units=97, seed=0, n_a_units=None):
    """layout: (lab, pairs, kind) in sorted order; kind "rand" (normal values), "lattice" (small integers: long tie
    groups), "equal" (one value), "one" (pairs of cohort A only), "drop" (lab -1: dropped pairs -- in turn of lab -1, of
    lab n_seg, of a unit out of range, of a value that is not finite).  The pairs are shuffled: the sort has work to do."""
    rng = np.random.default_rng(seed)
    group = np.zeros(n_units, np.uint8)
    group[rng.permutation(n_units)[:n_units // 3 if n_a_units is None else n_a_units]] = 1
    in_a = np.flatnonzero(group == 1)
    v, s, u = [], [], []
    for lab, m, kind in layout:
        s.append(np.full(m, lab, np.int64))
        u.append(in_a[rng.integers(0, in_a.size, m)] if kind == "one" else rng.integers(0, n_units, m))
        v.append({"rand": rng.normal(0.5, 2.0, m), "one": rng.normal(0.0, 1.0, m), "equal": np.full(m, 1.25),
                  "lattice": rng.integers(-3, 4, m).astype(np.float64), "drop": rng.normal(0.5, 2.0, m)}[kind].astype(F32))
        if kind == "drop":
            s[-1][1::4] = n_seg
            s[-1][2::4], s[-1][3::4] = 4, 4
            u[-1][2::8], u[-1][6::8] = -2, n_units
            v[-1][3::8], v[-1][7::8] = np.nan, np.inf
    cat = lambda x, dt: np.concatenate(x).astype(dt) if x else np.zeros(0, dt)      # noqa: E731
    v, s, u = cat(v, F32), cat(s, np.int64), cat(u, np.int64)
    p = rng.permutation(v.size)
    return {"value": v[p], "seg": s[p], "unit": u[p], "group": group, "n_seg": n_seg}


def near_exact(c, T, seed):
    """per (replicate, lab, field): the sum in extended precision, the sum of the absolute terms, the number of terms"""
    assert np.finfo(LD).nmant >= 63, "numpy's long double has no 64-bit significand here"
    v, seg, unit, group, n_seg = c["value"], c["seg"], c["unit"], c["group"], c["n_seg"]
    ok = (seg >= 0) & (seg < n_seg) & (unit >= 0) & (unit < group.size) & np.isfinite(v)
    ok &= np.where(ok, group[np.where(ok, unit, 0)] <= 1, False)
    keep = np.flatnonzero(ok)
    v32 = v[keep] + F32(0)
    order = np.lexsort((v32, seg[keep]))
    K, V, Un = seg[keep][order], v32[order].astype(LD), unit[keep][order]
    R1 = len(T)
    ref, mag = np.zeros((R1, n_seg, 5), LD), np.zeros((R1, n_seg, 5), LD)
    nterm = np.zeros((n_seg, 5), np.int64)
    A = sh.host_labels(seed, Un, group, T, 0, R1 - 1)
    lo_of = np.searchsorted(K, np.arange(n_seg + 1))
    for s in range(n_seg):
        lo, hi = lo_of[s], lo_of[s + 1]
        if hi == lo:
            continue
        a, x = A[:, lo:hi], V[lo:hi]
        ca = np.cumsum(a, axis=1, dtype=np.int64)
        d = ca * (hi - lo) - np.arange(1, hi - lo + 1)[None, :] * ca[:, -1:]
        dv = np.concatenate((x[1:] - x[:-1], [LD(0)]))
        w = np.abs(d).astype(LD) * dv[None, :]
        terms = (w, np.where(a, x, 0), np.where(a, 0, x), np.where(a, x * x, 0), np.where(a, 0, x * x))
        for f, t in enumerate(terms):
            ref[:, s, f], mag[:, s, f] = t.sum(axis=1), np.abs(t).sum(axis=1)
        nterm[s] = [np.count_nonzero(dv), hi - lo, hi - lo, hi - lo, hi - lo]
    return ref, mag, nterm


def to_dev(c, itype):
    d = lambda k, dt: torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV, dt)      # noqa: E731
    return d("value", torch.float32), d("seg", itype), d("unit", itype), d("group", torch.uint8)


def run_device(c, R, seed, itype):
    """the four calls into NaN / -1-filled outputs: an element a call does not write cannot pass"""
    v, seg, unit, group = to_dev(c, itype)
    n_seg = c["n_seg"]
    full = lambda shape, val, dt: torch.full(shape, val, dtype=dt, device=DEV)      # noqa: E731
    T, cohort = so.shift_thresholds(group, R, seed, out=(full((R + 1,), -1, torch.int64), full((3,), -1, torch.int64)))
    counts, sums, dropped = so.shift_stats(v, seg, unit, group, n_seg, T, seed, out=(
        full((R + 1, n_seg, 4), -1, torch.int64), full((R + 1, n_seg, 5), float("nan"), torch.float64),
        full((4,), -1, torch.int64)))
    stats = so.shift_finish(counts, sums, cohort, out=full((R + 1, n_seg + 1, 6), -7.0, torch.float64))
    summary = so.shift_summary(stats, out=full((n_seg + 1, 7), -7.0, torch.float64))
    return T, cohort, counts, sums, dropped, stats, summary


def check_case(c, R, seed, itype):
    T, cohort, counts, sums, dropped, stats, summary = run_device(c, R, seed, itype)
    wT, wc = sh.host_thresholds(c["group"], R, seed)
    assert same(cohort, wc) and wc[2] == 0
    gT = T.cpu().numpy().view(np.uint64)
    assert same(gT, wT), "the thresholds are not numpy.partition's"
    # the package's restatement EQUALS the loop reference (test_shift_cpu.py); here the device EQUALS the restatement
    w_counts, w_sums, w_dropped = sh.host_stats(c["value"], c["seg"], c["unit"], c["group"], c["n_seg"], wT, seed)
    assert same(dropped, w_dropped)
    g_counts, g_sums = counts.cpu().numpy(), sums.cpu().numpy()
    assert same(g_counts, w_counts), "n_a, n_b, K_plus, K_minus are exact"
    ref, mag, nterm = near_exact(c, wT, seed)
    bound = (nterm[None] + 8) * LD(U53) * mag - 3 * (nterm[None] + 1) * LD(2.0) ** -64 * mag
    err = np.abs(g_sums.astype(LD) - ref)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))) if err.size else 0.0
    print(f"n {len(c['value'])} R {R} n_seg {c['n_seg']}: largest |device - exact| / bound = {ratio:.3g}; "
          f"device == restatement bitwise: {same(g_sums, w_sums)}")
    assert (err <= bound).all()
    assert same(g_sums, w_sums), "the device and the restatement add the same terms in the same documented order"
    assert same(stats, sh.host_finish(g_counts, g_sums, wc)), "finish differs from the restatement on the device's tables"
    g_stats = stats.cpu().numpy()
    assert same(summary, sh.host_summary(g_stats)), "summary differs from the restatement on the device's statistics"
    return g_counts, g_sums, g_stats, summary.cpu().numpy()


# ---------------------------------------------------------------------------------- chunk sizes
LAYOUTS = {
    0: [],
    1: [(2, 1, "rand")],
    C - 1: [(0, 5, "rand"), (2, 200, "equal"), (3, 30, "one"), (5, C - 1 - 235, "rand")],
    C: [(0, 37, "rand"), (2, C - 37, "rand")],                                 # lab 2 ends exactly on the chunk's end
    C + 1: [(0, 60, "rand"), (2, C - 60, "lattice"), (4, 1, "rand")],          # ... and a pair follows in the next chunk
    2 * C + 3: [(0, 100, "rand"), (2, 2 * C - 98, "rand"), (3, 1, "one")],     # lab 2 spans three chunks
    # where k_sh_walk and k_sh_combine must agree on who writes a lab (SegChunks, csrc/segsort.h), with dropped pairs last
    C + 5: [(0, 37, "rand"), (2, C - 37, "rand"), (-1, 5, "drop")],            # ... and only dropped pairs follow
    490: [(0, 100, "rand"), (2, 300, "lattice"), (3, 50, "rand"), (-1, 40, "drop")],   # 2 direct; 3 mid-chunk, last kept: TAIL
    C + 10: [(5, 10, "rand"), (-1, C, "drop")],                                # a whole chunk without a kept pair
    7: [(-1, 7, "drop")],                                                      # no kept pair at all: zeros everywhere
}
ORDER = [0, 1, C - 1, C, C + 1, 2 * C + 3, C + 5, 490, C + 10, 7]             # a layout's seed and index width


@pytest.mark.parametrize("n", sorted(LAYOUTS))
def test_tables_finish_summary_at_every_chunk_count(n):
    i = ORDER.index(n)
    c = make_case(LAYOUTS[n], 6, seed=n)
    assert len(c["value"]) == n
    counts, sums, stats, _ = check_case(c, 5, 11 + i, torch.int64 if i % 2 else torch.int32)
    if n == 7:
        assert not counts.any() and not sums.any(), "all pairs dropped"
    tot = counts[0, :, 0] + counts[0, :, 1]
    assert tot.tolist() == [sum(m for lab, m, _ in LAYOUTS[n] if lab == s) for s in range(6)]
    assert tot[1] == 0 and not counts[:, 1].any() and not sums[:, 1].any(), "the empty lab between two filled ones"
    assert np.isnan(stats[:, 1, :5]).all()
    if n == C - 1:
        assert (counts[0, 3, 1] == 0) and np.isnan(stats[0, 3, :5]).all(), "a lab with pairs of one cohort only"
        assert not counts[:, 2, 2:].any() and not sums[:, 2, 0].any(), "all values equal: one tie group, D = W = 0"
        assert (stats[:, 2, 0] == 0).all()


def test_many_small_labs_inside_a_chunk_and_the_lab_limit():
    """2048 labs over C + 300 pairs: most labs begin and end inside a chunk and are written straight to the tables."""
    rng = np.random.default_rng(3)
    n, n_seg = C + 300, so.SHIFT_MAX_SEG
    c = {"value": rng.normal(size=n).astype(F32), "seg": np.minimum((rng.random(n) ** 2 * n_seg).astype(np.int64), n_seg - 1),
         "unit": rng.integers(0, 50, n), "group": (np.arange(50) % 2).astype(np.uint8), "n_seg": n_seg}
    counts, _, _, _ = check_case(c, 3, 4, torch.int64)
    assert ((counts[0, :, 0] + counts[0, :, 1]) == 0).any()


# ---------------------------------------------------------------------------------- tie groups and dropped pairs
@pytest.mark.parametrize("itype", [torch.int32, torch.int64])
def test_tie_groups_across_a_chunk_boundary_signed_zeros_and_dropped_pairs(itype):
    n = C + 500
    c = make_case([(0, n, "lattice")], 2, n_units=40, seed=5)              # 7 values: a tie group straddles position C
    c["group"][:2] = (2, 1)
    rng = np.random.default_rng(6)
    idx = rng.permutation(n)[:60]
    zeros = np.flatnonzero(c["value"] == 0)
    c["value"][zeros[::2]] = -0.0                                          # -0.0 beside +0.0: one tie group
    c["unit"][idx[50:60]] = 1                                              # (kept: these stay in range and finite)
    c["seg"][idx[:5]], c["seg"][idx[5:10]] = -1, 2
    c["unit"][idx[10:15]], c["unit"][idx[15:20]] = -2, 40
    c["unit"][idx[3]] = 40                                                 # lab and unit: counted under the lab
    c["value"][idx[20:25]], c["value"][idx[25:30]], c["value"][idx[30:35]] = np.nan, np.inf, -np.inf
    c["value"][idx[12]] = np.nan                                           # unit and value: counted under the unit
    c["unit"][idx[35:45]] = 0                                              # a unit whose group is 2
    g_of = c["group"][np.clip(c["unit"], 0, 39)]
    plain = np.ones(n, bool)
    plain[idx[:45]] = False
    n_group2 = 10 + int(np.count_nonzero(plain & (g_of == 2)))
    counts, sums, stats, _ = check_case(c, 9, 7, itype)
    T, cohort, _, _, dropped, _, _ = run_device(c, 9, 7, itype)
    assert dropped.tolist() == [10, 10, 15, n_group2]
    assert counts[0, 0, 0] + counts[0, 0, 1] == n - 35 - n_group2 > C, "the kept pairs of lab 0 reach past the chunk"
    # the signed zeros change nothing: the same case with +0.0 everywhere is bitwise the same
    c2 = dict(c, value=np.where(c["value"] == 0, F32(0), c["value"]))
    again = run_device(c2, 9, 7, itype)
    for a, b in zip(again[2:], run_device(c, 9, 7, itype)[2:]):
        assert torch.equal(bits(a), bits(b))
    # the dropped pairs are absent from every replicate: the case without them is bitwise the same
    ok = np.ones(n, bool)
    ok[idx[:45]] = False
    ok &= g_of <= 1
    c3 = {k: (x[ok] if k in ("value", "seg", "unit") else x) for k, x in c.items()}
    clean = run_device(c3, 9, 7, itype)
    assert not clean[4].any().item()
    for a, b in zip(clean[2:4] + clean[5:], again[2:4] + again[5:]):
        assert torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------- replicates and units
@pytest.mark.parametrize("R", [0, 1, RB - 1, RB, RB + 1])
def test_tables_finish_summary_at_every_replicate_block_count(R):
    c = make_case([(0, 300, "rand"), (1, 250, "lattice"), (2, 150, "rand")], 3, n_units=211, seed=R)
    _, _, _, summary = check_case(c, R, 2 ** 63 - 1 if R == RB else R, torch.int64)
    if R == 0:
        assert (summary[:3, :5] == 1).all() and summary[3, 4] == 1, "no replicate: every p-value is 1 / 1"


@pytest.mark.parametrize("n_units", [2, 3, 257])
@pytest.mark.parametrize("side", ["one_in_a", "one_in_b"])
def test_cohort_sizes_at_their_limits(n_units, side):
    n_a = 1 if side == "one_in_a" else n_units - 1
    c = make_case([(0, 400, "rand"), (1, 300, "lattice")], 2, n_units=n_units, seed=n_units, n_a_units=n_a)
    R = 40
    T, cohort, counts, *_ = run_device(c, R, 3, torch.int64)
    assert cohort.tolist() == [n_units, n_a, 0]
    check_case(c, R, 3, torch.int64)
    keys = np.stack([sh.unit_keys(3, b, np.arange(n_units)) for b in range(1, R + 1)])
    labels = keys <= T.cpu().numpy().view(np.uint64)[1:, None]
    assert (labels.sum(axis=1) == n_a).all(), "every replicate labels exactly U_A units as A"


def test_cohorts_without_a_unit_are_a_status_word_and_a_python_error():
    c = make_case([(0, 50, "rand")], 1, n_units=5, seed=1, n_a_units=0)
    for group in (np.zeros(5, np.uint8), np.ones(5, np.uint8), np.full(5, 2, np.uint8)):
        c["group"] = group
        T, cohort, *_ = run_device(c, 4, 0, torch.int64)             # every output is still written
        assert cohort[2].item() == so.SHIFT_BAD_COHORTS and not T.any().item()
        v, seg, unit, g = to_dev(c, torch.int64)
        with pytest.raises(ValueError, match="cohort"):
            sh.two_sample(v, seg, unit, g, 1, replicates=4)


def test_the_pair_is_the_unit_when_no_units_are_given():
    rng = np.random.default_rng(8)
    n = C + 77
    v = rng.normal(size=n).astype(F32)
    seg = rng.integers(0, 3, n)
    group = (rng.random(n) < 0.4).astype(np.uint8)
    v[group == 1] += F32(0.1) * (seg[group == 1] == 1)
    d = lambda x, dt: torch.from_numpy(x).to(DEV, dt)      # noqa: E731
    got = sh.two_sample(d(v, torch.float32), d(seg, torch.int64), None, d(group, torch.uint8), 3, replicates=60, seed=2,
                        return_replicates=True)
    want = sh.two_sample(v, seg, None, group, 3, replicates=60, seed=2, return_replicates=True)
    assert same(got.replicates["T"].cpu().numpy().view(np.uint64), want.replicates["T"])
    assert same(got.replicates["counts"], want.replicates["counts"])
    assert got.overall["n_units"] == n and got.dropped == want.dropped
    frames_agree(got.per_lab, want.per_lab, want.replicates, 60)


def frames_agree(got: pd.DataFrame, want: pd.DataFrame, tables, R):
    """integers and p-value counts EQUAL; floats inside the bounds the sums' bound gives them"""
    assert list(got.columns) == sh.COLUMNS == list(want.columns)
    for col in ("lab", "n_a", "n_b", "ks", "ks_signed", "p_ks", "p_adjusted", "p_asymptotic", "coverage_diff", "p_coverage"):
        assert same(got[col].to_numpy(), want[col].to_numpy()), col       # functions of the integer tables alone
    n = (want["n_a"] + want["n_b"]).to_numpy().astype(np.float64)
    rel = (n + 8) * U53 * 4
    g, w = got["wasserstein"].to_numpy(), want["wasserstein"].to_numpy()
    # W1 = W / P: the sum's bound relative to the sum of its (non-negative) terms, which is W itself, + the quotient
    assert np.all((np.abs(g - w) <= rel * np.abs(w)) | (np.isnan(g) & np.isnan(w)))
    # the p-values of W1 and smd move by 1 / (R + 1) per replicate whose statistic lies within rounding of replicate 0's
    st = np.asarray(tables["stats"].cpu() if torch.is_tensor(tables["stats"]) else tables["stats"])
    for col, f in (("p_wasserstein", 2), ("p_smd", 3)):
        x = np.abs(st[:, :len(n), f])
        close = (np.abs(x[1:] - x[0]) <= 1e-9 * np.abs(x[0])).sum(axis=0)
        assert np.all((np.abs(got[col].to_numpy() - want[col].to_numpy()) <= (close + 1e-9) / (R + 1))
                      | (np.isnan(got[col].to_numpy()) & np.isnan(want[col].to_numpy()))), col
    g, w = got["smd"].to_numpy(), want["smd"].to_numpy()
    assert np.all((np.abs(g - w) <= 1e-9 * np.maximum(np.abs(w), 1e-3)) | (np.isnan(g) & np.isnan(w)))


# ---------------------------------------------------------------------------------- determinism and capture
def test_three_eager_runs_and_three_replays_of_a_captured_graph_are_bitwise_equal():
    c = make_case([(0, 100, "rand"), (2, 2 * C - 98, "lattice"), (3, 1, "one")], 4, n_units=300, seed=21)
    R = RB + 1
    v, seg, unit, group = to_dev(c, torch.int64)

    def run():
        T, cohort = so.shift_thresholds(group, R, 17)
        counts, sums, dropped = so.shift_stats(v, seg, unit, group, 4, T, 17)
        stats = so.shift_finish(counts, sums, cohort)
        return T, cohort, counts, sums, dropped, stats, so.shift_summary(stats)

    first = [o.clone() for o in run()]
    for _ in range(2):
        for o, e in zip(run(), first):
            assert torch.equal(bits(o), bits(e)), "two eager runs differ"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                      # warm-up off the default stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for _ in range(3):
        for o in outs:
            o.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, first):
            assert torch.equal(bits(o), bits(e)), "a replayed capture differs from the eager run"


# ---------------------------------------------------------------------------------- refusals
def test_every_refusal_raises_and_leaves_the_outputs_untouched():
    c = make_case([(0, 100, "rand")], 3, n_units=10)
    v, seg, unit, group = to_dev(c, torch.int64)
    n = 100

    def filled(*shape, dtype=torch.float64):
        return torch.full(shape, -7, dtype=dtype, device=DEV)

    def untouched(*ts):
        torch.cuda.synchronize()
        return all(bool((t == -7).all()) for t in ts)

    T, cohort = so.shift_thresholds(group, 4, 0)
    for n_seg, R in ((3, -1), (3, so.SHIFT_MAX_REPLICATES + 1), (0, 4), (so.SHIFT_MAX_SEG + 1, 4)):
        assert so.load().mmg_shift_stats_ws_bytes(n, n_seg, R) == 0
        counts, sums, dropped = filled(5, 3, 4, dtype=torch.int64), filled(5, 3, 5), filled(4, dtype=torch.int64)
        with pytest.raises(MmgError, match="replicates|segments"):
            so._call("mmg_shift_stats", v, ops._p(seg, torch.int64), ops._p(unit, torch.int64), 8, n, n_seg, group, 10, R, 0, T,
                     counts, sums, dropped, ws=1 << 20)
        st, sm = filled(5, 4, 6), filled(4, 7)
        with pytest.raises(MmgError, match="replicates|segments"):
            so._call("mmg_shift_finish", counts, sums, cohort, n_seg, R, st)
        with pytest.raises(MmgError, match="replicates|segments"):
            so._call("mmg_shift_summary", st, n_seg, R, sm)
        assert untouched(counts, sums, dropped, st, sm)
    Tf, cf_ = filled(5, dtype=torch.int64), filled(3, dtype=torch.int64)
    for R in (-1, so.SHIFT_MAX_REPLICATES + 1):
        with pytest.raises(MmgError, match="replicates"):
            so._call("mmg_shift_thresholds", group, 10, R, 0, Tf, cf_)
    with pytest.raises(MmgError, match="units"):
        so._call("mmg_shift_thresholds", group, -1, 4, 0, Tf, cf_)
    with pytest.raises(MmgError, match="null"):
        so._call("mmg_shift_thresholds", None, 10, 4, 0, Tf, cf_)
    with pytest.raises(MmgError, match="null"):
        so._call("mmg_shift_thresholds", group, 10, 4, 0, None, cf_)
    assert untouched(Tf, cf_)
    counts, sums, dropped = filled(5, 3, 4, dtype=torch.int64), filled(5, 3, 5), filled(4, dtype=torch.int64)
    ws = ops.workspace(so.load().mmg_shift_stats_ws_bytes(n, 3, 4), DEV)
    args = [v, ops._p(seg, torch.int64), ops._p(unit, torch.int64), 8, n, 3, group, 10, 4, 0, T, counts, sums, dropped]

    def with_(i, x):
        a = list(args)
        a[i] = x
        return a

    with pytest.raises(MmgError, match="index_bytes"):
        so._call("mmg_shift_stats", *with_(3, 2), ws=ws)
    for i in (0, 1, 2, 6, 10, 11, 12, 13):                         # null value, seg, unit, group, T, counts, sums, dropped
        with pytest.raises(MmgError, match="null"):
            so._call("mmg_shift_stats", *with_(i, None), ws=ws)
    with pytest.raises(MmgError, match="units"):
        so._call("mmg_shift_stats", *with_(7, -1), ws=ws)
    with pytest.raises(MmgError, match="outside"):
        so._call("mmg_shift_stats", *with_(4, -1), ws=ws)
    with pytest.raises(MmgError, match="workspace"):
        so._call("mmg_shift_stats", *args, ws=torch.empty(1024, dtype=torch.uint8, device=DEV))
    with pytest.raises(MmgError, match="workspace"):
        so._call("mmg_shift_stats", *args)                         # no workspace at all
    assert untouched(counts, sums, dropped)
    st, sm = filled(5, 4, 6), filled(4, 7)
    with pytest.raises(MmgError, match="null"):
        so._call("mmg_shift_finish", counts, sums, None, 3, 4, st)
    with pytest.raises(MmgError, match="null"):
        so._call("mmg_shift_summary", None, 3, 4, sm)
    assert untouched(st, sm)
    with pytest.raises(TypeError):
        sh.shift_tables(v, c["seg"], c["unit"], c["group"], 3, 4)                      # device and host inputs mixed
    with pytest.raises(MmgError):
        so.shift_summary(torch.zeros(5, 4, 6, dtype=torch.float64))                    # a host tensor: no fallback


# ---------------------------------------------------------------------------------- drivers
@pytest.fixture(scope="module")
def trained():
    from mmgnn import conformal as cf
    g = make_graph(1, seed=0).to(DEV)
    cfg = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.0,
                     "use_batch_norm": True, "activation": "relu"}}
    torch.manual_seed(0)
    model = build_model(cfg, (g.node_types, g.edge_types), None).to(DEV)
    model._init_embeddings(g)
    masker = EdgeMasker(g)
    pi, li, y = cf._split_pairs(g, masker, "train")
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    model.train()
    for _ in range(5):                                       # briefly trained
        opt.zero_grad()
        (model.predict_lab_values(g, pi, li).reshape(-1) - y).abs().mean().backward()
        opt.step()
    return g, model, masker


def host_args(args):
    return [None if a is None else a.cpu().numpy() for a in args]


@pytest.mark.parametrize("splitter", ["edge", "patient"])
def test_split_shift_equals_the_numpy_path_on_the_same_pairs(trained, tmp_path, splitter):
    from mmgnn import conformal as cf
    g, _, masker = trained
    if splitter == "patient":
        masker = PatientHoldoutSplitter(g)
    R = 50
    res = sh.split_shift(g, masker, output_dir=tmp_path, replicates=R, seed=1, return_replicates=True)
    assert (tmp_path / "split_shift.csv").exists()
    assert list(pd.read_csv(tmp_path / "split_shift.csv").columns) == sh.COLUMNS
    a, b = cf._split_pairs(g, masker, "train"), cf._split_pairs(g, masker, "test")
    args = sh._two_splits(a, b, int(g["patient"].num_nodes), splitter == "patient")
    n_labs = int(g["lab"].num_nodes)
    want = sh.two_sample(*host_args(args), n_labs=n_labs, replicates=R, seed=1, return_replicates=True)
    assert (args[2] is None) == (splitter == "edge")
    assert res.overall["n_units"] == want.overall["n_units"] and res.dropped == want.dropped
    assert same(res.replicates["counts"], want.replicates["counts"])
    assert same(res.replicates["summary"][:, 5:], want.replicates["summary"][:, 5:]), "the p-value counts"
    frames_agree(res.per_lab, want.per_lab, want.replicates, R)
    assert res.overall["max_z"] == want.overall["max_z"] and res.overall["p"] == want.overall["p"]


def test_residual_shift_equals_the_numpy_path_on_the_same_pairs(trained, tmp_path):
    from mmgnn import conformal as cf
    g, model, masker = trained
    R = 50
    res = sh.residual_shift(model, g, masker, output_dir=tmp_path, replicates=R, seed=2, return_replicates=True)
    assert (tmp_path / "residual_shift.csv").exists() and not (tmp_path / "split_shift.csv").exists()
    out = []
    for split in ("val", "test"):
        _, pred, y, pi, li = cf._predict_split(model, g, masker, split)
        out.append((pi, li, pred - y))
    args = sh._two_splits(out[0], out[1], int(g["patient"].num_nodes), False)
    want = sh.two_sample(*host_args(args), n_labs=int(g["lab"].num_nodes), replicates=R, seed=2, return_replicates=True)
    assert same(res.replicates["counts"], want.replicates["counts"])
    assert same(res.replicates["summary"][:, 5:], want.replicates["summary"][:, 5:]), "the p-value counts"
    frames_agree(res.per_lab, want.per_lab, want.replicates, R)
    assert res.overall["shifted_labs"] == want.overall["shifted_labs"]

    class Sharded:
        _comm = object()

    for call in (lambda: sh.residual_shift(Sharded(), g, masker), lambda: sh.split_shift(g, masker, model=Sharded()),
                 lambda: sh.triples_shift(out[0], out[1], 3, model=Sharded())):
        with pytest.raises(NotImplementedError):
            call()
